"""The device's random draws restated with numpy, so that a stream can be replayed: the hash and one twin per game's random
policy.  Every name here is also ``simulators``'.

May import: numpy, inside the functions (the package imports without it), and nothing of the package.
"""


def random_hash(seed, step, world, player):
    """The counter-based hash behind the device-side random policies (``mrl_rollout_random``;
    csrc/random_policy.hpp), restated with numpy so a stream can be replayed.  uint32 array."""
    import numpy as np
    m = np.uint64(0xFFFFFFFF)
    seed = int(seed) & (2 ** 64 - 1)
    h = (np.uint64(seed & 0xFFFFFFFF) ^ (np.uint64(step) * np.uint64(0x9E3779B9) & m) ^
         (np.asarray(world, np.uint64) * np.uint64(0x85EBCA6B) & m) ^
         ((np.asarray(player, np.uint64) + np.uint64(1)) * np.uint64(0xC2B2AE35) & m) ^
         (np.uint64(seed >> 32) * np.uint64(0x27D4EB2F) & m))
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x7FEB352D) & m
    h ^= h >> np.uint64(15)
    h = h * np.uint64(0x846CA68B) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def sample_u(seed, step, world):
    """The uniform number behind ``rollout_policy``'s draw for (step index, world): ``(hash >> 8) * 2^-24`` with player 0,
    a multiple of 2^-24 in [0, 1) and exact in float32 (``mrl_rollout_policy``).  float32 array."""
    import numpy as np
    h = random_hash(seed, step, world, np.zeros_like(np.asarray(world)))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def random_action(seed, step, world, player):
    """Overcooked: ``(hash * 6) >> 32`` for (step index, world, player)."""
    import numpy as np
    return ((random_hash(seed, step, world, player).astype(np.uint64) * np.uint64(6)) >> np.uint64(32)).astype(np.int32)


def random_cartpole_action(seed, step, world):
    """Cartpole: the hash's top bit (player 0)."""
    import numpy as np
    return (random_hash(seed, step, world, np.zeros_like(np.asarray(world))) >> np.uint32(31)).astype(np.int32)


def random_acrobot_action(seed, step, world):
    """Acrobot: ``(hash * 3) >> 32`` for (step index, world, player 0)."""
    import numpy as np
    h = random_hash(seed, step, world, np.zeros_like(np.asarray(world)))
    return ((h.astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int32)


def random_hanabi_action(seed, step, world, mover, legal_mask):
    """Hanabi: the k-th legal move of the mover, ``k = (hash * count) >> 32``.
    ``legal_mask``: (n, 20) 0/1 array of the mover's legal moves, ``mover``: (n,) 0/1."""
    import numpy as np
    legal_mask = np.asarray(legal_mask) != 0
    count = legal_mask.sum(-1).astype(np.uint64)
    k = (random_hash(seed, step, world, mover).astype(np.uint64) * count) >> np.uint64(32)
    rank = np.cumsum(legal_mask, axis=-1) - 1                      # rank of each legal move among the legal ones
    pick = legal_mask & (rank == k[:, None].astype(np.int64))
    return np.where(count > 0, pick.argmax(-1), 0).astype(np.int32)


def random_balance_action(seed, step, world, player):
    """Balance beam: ``(hash * 4) >> 32`` for (step index, world, player)."""
    import numpy as np
    return ((random_hash(seed, step, world, player).astype(np.uint64) * np.uint64(4)) >> np.uint64(32)).astype(np.int32)

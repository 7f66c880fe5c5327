"""What the GPU tests of the MAPPO policy banks (test_gpu_cnn_bank.py, test_gpu_mlpbase_bank.py) share: reading tensors back,
comparing bits, the plan's workspace layout of include/mrl_envs.h and the assertions on a plan read back from it."""
import numpy as np


def cpu(t):
    return (t.to_torch() if hasattr(t, "to_torch") else t).cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def workspace_layout(n, p, k):
    cells, kp = n * p, (k + 3) // 4 * 4
    max_tiles = (cells + 31) // 32 + k
    table = 4 + 2 * kp
    return {"count": 4, "start": 4 + kp, "table": table, "lists": table + 4 * max_tiles, "max_tiles": max_tiles}


def assert_plan_read_back(block, size, n, p, k, ids, acted, out_of_range):
    """``block``: 256 guard bytes of 0xA5, the ``size`` bytes of the workspace after an act of ``n`` worlds of ``p`` seats under a
    bank of ``k``, guard bytes again; ``ids`` (N, P) as given, ``acted`` (N, P) the cells that had to act, ``out_of_range`` the
    masked ids beyond the bank."""
    assert (block[:256] == 0xA5).all() and (block[256 + size:] == 0xA5).all()  # the guard bytes
    words = block[256:256 + size].view(np.uint32)
    at = workspace_layout(n, p, k)
    tiles, n_acted, beyond = (int(x) for x in words[:3])
    assert n_acted == acted.sum() and beyond == out_of_range and words[3] == 0
    counts = words[at["count"]:at["count"] + k]
    starts = words[at["start"]:at["start"] + k]
    flat_ids, flat_acted = ids.reshape(-1), acted.reshape(-1)
    assert np.array_equal(counts, [(flat_acted & (flat_ids == j)).sum() for j in range(k)])
    assert np.array_equal(counts, np.bincount(flat_ids[flat_acted], minlength=k))
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(counts)[:-1]]))
    assert tiles == sum((int(cnt) + 31) // 32 for cnt in counts) <= (n * p + 31) // 32 + k == at["max_tiles"]
    lists = words[at["lists"]:at["lists"] + n_acted]
    # every acted cell once, in its own policy's list, ascending
    assert np.array_equal(np.sort(lists), np.flatnonzero(flat_acted))
    for j in range(k):
        mine = lists[starts[j]:starts[j] + counts[j]]
        assert np.array_equal(mine, np.flatnonzero(flat_acted & (flat_ids == j)))
    # tiles: one policy each, consecutive pieces of that policy's list, 32 rows but for the last
    table = words[at["table"]:at["table"] + 4 * tiles].reshape(tiles, 4)
    covered = np.zeros(n_acted, dtype=np.int32)
    for policy, first, rows, zero in table:
        assert 1 <= rows <= 32 and zero == 0 and policy < k
        assert starts[policy] <= first and first + rows <= starts[policy] + counts[policy]
        assert (flat_ids[lists[first:first + rows]] == policy).all()
        covered[first:first + rows] += 1
    assert (covered == 1).all()
    assert np.array_equal(np.bincount(table[:, 0], minlength=k), [(int(cnt) + 31) // 32 for cnt in counts])

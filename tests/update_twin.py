"""What ``ppo_twin`` and ``mappo_twin`` share: ``clip_grad_norm_`` and Adam in float64 numpy and through torch's own classes --
the arithmetic the device's optimiser tail (csrc/adam_step.hpp) must match --, and the helpers of both updates' cases.  Nothing
here touches a GPU."""
import numpy as np
import torch


def f32(x):
    return float(np.float32(x))


def clip_adam(params, exp_avg, exp_avg_sq, grad, step, max_grad_norm, lr, cfg):
    """clip_grad_norm_ and one torch.optim.Adam step (single tensor, no amsgrad, no weight decay) over one flat array in float64
    numpy; ``step``: steps taken before; ``max_grad_norm`` None: no clipping; ``cfg`` gives beta1, beta2 and eps.  Returns
    (total_norm, params, exp_avg, exp_avg_sq)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (params, exp_avg, exp_avg_sq, grad))
    total = float(np.sqrt(np.sum(g * g)))
    if max_grad_norm is not None:
        g = g * min(1.0, max_grad_norm / (total + 1e-6))
    t = step + 1
    m = cfg.beta1 * m + (1 - cfg.beta1) * g
    v = cfg.beta2 * v + (1 - cfg.beta2) * g * g
    p = p - (lr / (1 - cfg.beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - cfg.beta2 ** t) + cfg.eps)
    return total, p, m, v


def clip_adam_torch(params, exp_avg, exp_avg_sq, grad, step, max_grad_norm, lr, cfg, dtype=torch.float64):
    """The same through ``clip_grad_norm_`` and ``torch.optim.Adam`` themselves on one flat CPU tensor of ``dtype`` (copies: the
    caller's arrays stay as they are)."""
    p = torch.nn.Parameter(torch.tensor(np.asarray(params, np.float64)).to(dtype))
    p.grad = torch.tensor(np.asarray(grad, np.float64)).to(dtype)
    total = float(torch.linalg.vector_norm(p.grad).item())
    if max_grad_norm is not None:
        total = float(torch.nn.utils.clip_grad_norm_([p], max_grad_norm).item())
    opt = torch.optim.Adam([p], lr=lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(np.asarray(exp_avg, np.float64)).to(dtype),
                    "exp_avg_sq": torch.tensor(np.asarray(exp_avg_sq, np.float64)).to(dtype)}
    opt.step()
    state = opt.state[p]
    return total, p.detach().double().numpy(), state["exp_avg"].double().numpy(), state["exp_avg_sq"].double().numpy()


def moments(num_params, seed):
    """Adam moments of a run in progress (float32): exp_avg of the size of a gradient, exp_avg_sq of its square."""
    rng = np.random.default_rng(seed)
    return (rng.normal(scale=1e-2, size=num_params).astype(np.float32),
            (rng.normal(scale=1e-2, size=num_params) ** 2 + 1e-8).astype(np.float32))


def make_indices(rows, width, size, seed):
    """(rows, width) int32 sample numbers below ``size``, each row without repeats -- or, wider than the batch, drawn with them"""
    rng = np.random.default_rng(seed + 1)
    if width > size:
        return rng.integers(0, size, size=(rows, width)).astype(np.int32)
    return np.stack([rng.permutation(size)[:width] for _ in range(rows)]).astype(np.int32)


def distance(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def tile_size(workspace_bytes):
    """The gradient kernel's tile, read off ``workspace_bytes(B)``: the largest B that still needs one partial vector."""
    base = workspace_bytes(1)
    width = 1
    while workspace_bytes(width + 1) == base:
        width += 1
        assert width < 1 << 16
    return width


def saturation(workspace_bytes):
    """(tile, cap * tile): the gradient kernel's tile and the cap on partial vectors times the tile, the largest B at which every
    workgroup still takes a single tile.  ``workspace_bytes(B)`` reaches its final value where the last of those tiles begins."""
    tile = tile_size(workspace_bytes)
    top = workspace_bytes((1 << 31) - 1)
    low, high = 1, (1 << 31) - 1
    while low < high:
        mid = (low + high) // 2
        if workspace_bytes(mid) == top:
            high = mid
        else:
            low = mid + 1
    return tile, low - 1 + tile

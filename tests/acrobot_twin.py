"""TEST ONLY -- the Acrobot step in float64 numpy: the reference's program (src/acrobat_env/sim.cpp:68-206) evaluated
without rounding.  The constants are the values the reference HOLDS -- its pi, g, dt and dt / 6 are floats -- so what
separates a float32 implementation from this twin is its own rounding and its sin / cos, nothing else.  Angles are
wrapped fully (one piece, however far), velocities clamped; ``raw`` keeps the velocities before the clamp."""
import numpy as np

PI_F = float(np.float32(np.pi))              # madrona::math::pi
G = float(np.float32(9.8))
DT = float(np.float32(0.2))
DT2 = float(np.float32(DT / 2.0))            # float dt2 = dt / 2.0
DT6 = float(np.float32(DT / 6.0))            # float dt6 = dt / 6.0
MAX_VEL_1 = float(np.float32(4) * np.float32(np.pi))
MAX_VEL_2 = float(np.float32(9) * np.float32(np.pi))
HALF_PI = PI_F / 2.0
MAX_STEPS = 500


def derivs(y, a):
    t1, t2, w1, w2 = y[..., 0], y[..., 1], y[..., 2], y[..., 3]
    c2, s2 = np.cos(t2), np.sin(t2)
    d1 = 0.25 + (1.25 + c2) + 2.0
    d2 = 0.25 + 0.5 * c2 + 1.0
    phi2 = 0.5 * G * np.cos(t1 + t2 - HALF_PI)
    phi1 = -0.5 * w2 * w2 * s2 - w2 * w1 * s2 + 1.5 * G * np.cos(t1 - HALF_PI) + phi2
    dw2 = (a + d2 / d1 * phi1 - 0.5 * w1 * w1 * s2 - phi2) / (1.25 - d2 * d2 / d1)
    dw1 = -(d2 * dw2 + phi1) / d1
    return np.stack([w1, w2, dw1, dw2], axis=-1)


def wrap(x):
    two_pi = 2.0 * PI_F
    x = np.where(x > PI_F, x - two_pi * np.ceil((x - PI_F) / two_pi), x)
    return np.where(x < -PI_F, x + two_pi * np.ceil((-PI_F - x) / two_pi), x)


def step(state, action, detail=False):
    """state (n, 4), action (n,) in {0, 1, 2} -> (next state (n, 4) float64, height (n,), raw velocities (n, 2)); with
    ``detail`` also the new angles before the wrap (n, 2) and the largest |angle| any of the four stages evaluates (n,)."""
    y0 = np.asarray(state, np.float64)
    a = np.asarray(action, np.float64) - 1.0
    k1 = derivs(y0, a)
    y1 = y0 + k1 * DT2
    k2 = derivs(y1, a)
    y2 = y0 + k2 * DT2
    k3 = derivs(y2, a)
    y3 = y0 + k3 * DT
    k4 = derivs(y3, a)
    n = y0 + (k1 + 2.0 * k2 + 2.0 * k3 + k4) * DT6
    out = np.stack([wrap(n[:, 0]), wrap(n[:, 1]), np.clip(n[:, 2], -MAX_VEL_1, MAX_VEL_1),
                    np.clip(n[:, 3], -MAX_VEL_2, MAX_VEL_2)], axis=1)
    height = -np.cos(out[:, 0]) - np.cos(out[:, 1] + out[:, 0])
    if detail:
        reach = np.abs(np.stack([y0[:, :2], y1[:, :2], y2[:, :2], y3[:, :2]])).max(axis=(0, 2))
        return out, height, n[:, 2:4], n[:, 0:2], reach
    return out, height, n[:, 2:4]


def angle_distance(a, b):
    """|a - b| for angles, modulo the reference's 2 pi."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, np.abs(d - 2.0 * PI_F))


def distance(a, b):
    """per component |a - b| of two (n, 4) states, the angles modulo 2 pi"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([angle_distance(a[:, :2], b[:, :2]), np.abs(a[:, 2:] - b[:, 2:])], axis=1)

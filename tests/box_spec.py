"""The Box shape's rule (include/flux_abi.h flux_shape) in numpy, f64, operation for operation: the reference the
GPU tests compare against.  BoundingBox::hit's slabs (shapes.rs:99-131) with the reference's own max / min, whose NaN behaviour is
part of the rule; the hit is the entry if it lies beyond T_MIN, else the exit; the face is the first axis whose own bound is t."""
import numpy as np

T_MIN = 0.0005  # constants.rs:4


def ref_max(a, b):
    """shapes.rs:90-92: if a > b {a} else {b} -- a NaN `a` is dropped, a NaN `b` comes out."""
    return np.where(a > b, a, b)


def ref_min(a, b):
    """shapes.rs:94-96: if a < b {a} else {b}."""
    return np.where(a < b, a, b)


def slabs(c0, c1, o, d):
    """(tmin[n, 3], tmax[n, 3], a[n, 3]) of rays o, d ([n, 3]) against the box c0, c1."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = 1.0 / d
        lo = (np.asarray(c0, dtype=np.float64) - o) * a
        hi = (np.asarray(c1, dtype=np.float64) - o) * a
    pos = a >= 0.0
    return np.where(pos, lo, hi), np.where(pos, hi, lo), a


def box_hit(c0, c1, o, d, invert=False):
    """hit[n] (bool), t[n], normal[n, 3], face[n] (2 axis + 1 if the outward normal is +e_axis; -1 on a miss) and the
    intermediate (t0, t1, tmin, tmax) for the rounding-level exclusions of the tests."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    tmin, tmax, a = slabs(c0, c1, o, d)
    with np.errstate(invalid="ignore"):
        t0 = ref_max(tmin[:, 0], ref_max(tmin[:, 1], tmin[:, 2]))
        t1 = ref_min(tmax[:, 0], ref_min(tmax[:, 1], tmax[:, 2]))
        entry = t0 > T_MIN
        t = np.where(entry, t0, t1)
        hit = (t0 < t1) & (t > T_MIN)
        bound = np.where(entry[:, None], tmin, tmax)
        axis = np.where(bound[:, 0] == t, 0, np.where(bound[:, 1] == t, 1, 2))
    pos = a[np.arange(len(a)), axis] >= 0.0
    plus = entry != pos  # entry: -e if a >= 0; exit: the opposite
    face = np.where(hit, 2 * axis + plus, -1)
    n = np.zeros_like(o)
    n[np.arange(len(o)), axis] = np.where(plus, 1.0, -1.0) * (-1.0 if invert else 1.0)
    n[~hit] = 0.0
    return hit, np.where(hit, t, 0.0), n, face, (t0, t1, tmin, tmax)


def rounding_level(t0, t1, tmin, tmax, eps=1e-9):
    """Rays whose decision sits at rounding level (excluded from FAST comparisons, counted): |t - T_MIN|, |t0 - t1| or the two
    largest tmin (two smallest tmax) within `eps` relative."""
    with np.errstate(invalid="ignore"):
        def close(x, y):
            return np.isfinite(x) & np.isfinite(y) & (np.abs(x - y) <= eps * np.maximum(np.abs(x), np.abs(y)))
        lo = np.sort(np.where(np.isnan(tmin), -np.inf, tmin), axis=1)
        hi = np.sort(np.where(np.isnan(tmax), np.inf, tmax), axis=1)
        r = close(t0, T_MIN) | close(t1, T_MIN) | close(t0, t1)
        r |= close(lo[:, 2], lo[:, 1]) | close(hi[:, 0], hi[:, 1])
    return r


def brute_force(c0, c1, o, d, invert=False):
    """The same box as six bounded planes, evaluated independently: every face plane's t = (c - o_k) / d_k, kept if t > T_MIN and
    the hit point lies inside the face's rectangle (closed, with a hair of slack); nearest wins.  The entry / exit rule follows:
    from outside the nearest is the entry, from inside (or from a face, leaving inwards) the exit.  For rays that avoid ties."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    c = (np.asarray(c0, dtype=np.float64), np.asarray(c1, dtype=np.float64))
    best_t = np.full(len(o), np.inf)
    best_face = np.full(len(o), -1)
    for axis in range(3):
        for side in range(2):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (c[side][axis] - o[:, axis]) / d[:, axis]
                q = o + t[:, None] * d
            ok = np.isfinite(t) & (t > T_MIN)
            for other in range(3):
                if other != axis:
                    slack = 1e-12 * (1.0 + np.abs(c[0][other]) + np.abs(c[1][other]))
                    with np.errstate(invalid="ignore"):
                        ok &= (q[:, other] >= c[0][other] - slack) & (q[:, other] <= c[1][other] + slack)
            take = ok & (t < best_t)
            best_t = np.where(take, t, best_t)
            best_face = np.where(take, 2 * axis + side, best_face)
    hit = best_face >= 0
    n = np.zeros_like(o)
    n[np.arange(len(o)), np.maximum(best_face, 0) // 2] = np.where(best_face % 2 == 1, 1.0, -1.0) * (-1.0 if invert else 1.0)
    n[~hit] = 0.0
    return hit, np.where(hit, best_t, 0.0), n, best_face

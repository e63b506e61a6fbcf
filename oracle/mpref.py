"""High-precision references for the dense-algebra tests (mpmath, 50 significant digits, from the exact float32 inputs).

inverse6:     the inverse of a 6 x 6 matrix, and its 2-norm condition number from the symmetric eigenvalues.
pinv3_sym:    the Moore-Penrose pseudo-inverse of a packed symmetric 3 x 3 (xx, xy, xz, yy, yz, zz) under the rule of the device's
              per-voxel weight (icet_device_math.h pinv3_sym / pinv3_sym_fast): eigenvalues with |lambda| <= rel * max |lambda| are dropped.
"""
import numpy as np
import mpmath

DPS = 50
EPS_F = float(np.finfo(np.float32).eps)


def _mat(a):
    return mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in np.asarray(a, np.float64)])


def inverse6(H):
    """(inverse as float64 array, cond_2) of the float32 matrix H, both computed at DPS digits."""
    with mpmath.workdps(DPS):
        A = _mat(H)
        inv = A ** -1
        ev = mpmath.eigsy(A, eigvals_only=True)
        lam = sorted(abs(e) for e in ev)
        cond = float(lam[-1] / lam[0]) if lam[0] != 0 else float("inf")
        return np.array([[float(inv[i, j]) for j in range(6)] for i in range(6)]), cond


def unpack3(p):
    p = np.asarray(p, np.float64)
    return np.array([[p[0], p[1], p[2]], [p[1], p[3], p[4]], [p[2], p[4], p[5]]])


def pack_upper(A):
    A = np.asarray(A)
    return np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]], A.dtype)


def pinv3_sym(packed, rel=3 * EPS_F):
    """(W packed as float64 (6,), rank, cond of the kept eigenvalues) of the exact float32 input; rel: the relative rank threshold."""
    with mpmath.workdps(DPS):
        A = _mat(unpack3(packed))
        ev, Q = mpmath.eigsy(A)
        lmax = max(abs(e) for e in ev)
        keep = [k for k in range(3) if abs(ev[k]) > mpmath.mpf(rel) * lmax]
        W = mpmath.zeros(3, 3)
        for k in keep:
            for i in range(3):
                for j in range(3):
                    W[i, j] += Q[i, k] * Q[j, k] / ev[k]
        kept = [abs(ev[k]) for k in keep]
        cond = float(max(kept) / min(kept)) if kept else 1.0
        return np.array([float(W[0, 0]), float(W[0, 1]), float(W[0, 2]), float(W[1, 1]), float(W[1, 2]), float(W[2, 2])]), len(keep), cond

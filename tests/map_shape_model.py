"""A NumPy restatement of the voxel map's shape rule (include/icet_hip.h icet_voxel_map_enable_shape / extract_shape; the device compiles
icet_amd/csrc/icet_map_shape.h), on top of tests/map_model.py: the nine moment words per cell in Python integers, the covariance in the rule's expression order
with Python floats (IEEE double, one rounding per operation), and the cyclic Jacobi restated operation by operation."""
import math

import numpy as np

import map_model as mm

WORDS = 9                                                             # S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz
SWEEPS = 6
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
MASK = (1 << 64) - 1


def row_moments(q):
    """What each kept row adds: (N, 9) int64 from the (N, 3) offsets q of map_model.classify.  h = q >> 16; every entry is below 2^32."""
    h = (np.asarray(q, np.uint64) >> np.uint64(16)).astype(np.int64)
    return np.stack([h[:, 0], h[:, 1], h[:, 2]] + [h[:, a] * h[:, b] for a, b in PAIRS], axis=1)


def cov(n, words, cell):
    """The double C (xx, xy, xz, yy, yz, zz) of a cell of count n >= 1: m_a = S_a / n, E_ab = M_ab / n, C_ab = (E_ab - m_a m_b) k2, the words taken as uint64."""
    k = float(np.float32(cell)) * 2.0 ** -16
    k2 = k * k
    nd = float(int(n))
    m = [float(int(words[a]) & MASK) / nd for a in range(3)]
    return np.array([(float(int(words[3 + j]) & MASK) / nd - m[a] * m[b]) * k2 for j, (a, b) in enumerate(PAIRS)], np.float64)


def jacobi(C6, sweeps=SWEEPS):
    """The rule's cyclic Jacobi on one double C: (A, V) after ``sweeps`` sweeps, as nested lists of Python floats."""
    C = [float(v) for v in C6]
    A = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(sweeps):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            inv = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            t = -inv if theta < 0.0 else inv
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            ta = t * apq
            A[p][p] = A[p][p] - ta
            A[q][q] = A[q][q] + ta
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for i in range(3):
                vp, vq = V[i][p], V[i][q]
                V[i][p] = c * vp - s * vq
                V[i][q] = s * vp + c * vq
    return A, V


def eigen(C6):
    """(evals, normal), float32: the diagonal ascending by a stable sort, the column of the smallest (ties: the lowest column) rounded to float32 and signed so
    that its component of largest magnitude is positive, the lowest axis winning a tie."""
    A, V = jacobi(C6)
    d = [A[0][0], A[1][1], A[2][2]]
    order = sorted(range(3), key=lambda i: d[i])                      # (Python's sort is stable)
    v = np.array([V[i][order[0]] for i in range(3)], np.float64).astype(np.float32)
    j = 0
    if abs(v[1]) > abs(v[0]):
        j = 1
    if abs(v[2]) > abs(v[j]):
        j = 2
    if v[j] < 0:
        v = -v
    return np.array([d[i] for i in order], np.float64).astype(np.float32), v


def world_rows(scan, pose):
    """The rows of a scan in the world frame in float64, in the rule's expression order: ((R0 x + R1 y) + R2 z) + t."""
    p = np.asarray(scan, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], axis=1)


class ShapeMap(mm.Map):
    """map_model.Map, and per key the nine moment words as Python integers (two's complement is taken when they are read: words())."""

    def clear(self):
        super().clear()
        self.mom = {}

    def add(self, scans, poses, sign=1):
        super().add(scans, poses, sign)
        poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
        for scan, T in zip(scans, poses):
            cls, key, q, _ = mm.classify(scan, T, self.cell, self.min_range, self.max_range)
            keep = cls == mm.KEPT
            if not keep.any():
                continue
            uk, inv = np.unique(key[keep], return_inverse=True)
            tot = np.zeros((uk.shape[0], WORDS), np.int64)
            np.add.at(tot, inv, row_moments(q[keep]))                 # (a scan's rows x 2^32 stays far below 2^63)
            for i, k in enumerate(uk):
                e = self.mom.setdefault(int(k), [0] * WORDS)
                for w in range(WORDS):
                    e[w] += sign * int(tot[i, w])
        return self

    def words(self, key):
        return [w & MASK for w in self.mom[int(key)]]

    def extract_shape(self, min_points=1, cap_rows=None, eig=True):
        """extract's dict, and moments (n, 9) uint64, cov64 (n, 6) float64 (the rule's double C), cov (n, 6) float32, and with ``eig`` evals and normal (n, 3)
        float32."""
        res = self.extract(min_points, cap_rows)
        n = res["key"].shape[0]
        res["moments"] = np.array([self.words(k) for k in res["key"]], np.uint64).reshape(n, WORDS)
        res["cov64"] = np.array([cov(c, self.words(k), self.cell) for k, c in zip(res["key"], res["count"])], np.float64).reshape(n, 6)
        res["cov"] = res["cov64"].astype(np.float32)
        if not eig:
            return res
        eg = [eigen(C) for C in res["cov64"]]
        res["evals"] = np.array([e for e, _ in eg], np.float32).reshape(n, 3)
        res["normal"] = np.array([v for _, v in eg], np.float32).reshape(n, 3)
        return res


def cov_matrix(C6):
    C = np.asarray(C6)
    return C[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(C.shape[:-1] + (3, 3))


PLANE_NORMAL = np.array([-0.3, -0.1, 1.0]) / np.sqrt(0.3 ** 2 + 0.1 ** 2 + 1.0)


def plane_rows(n=60000, sigma=0.02, seed=7):
    """The plane z = 0.3 x + 0.1 y + 2 sampled at n uniform (x, y) in [0, 10]^2, with Gaussian noise of ``sigma`` along the normal: (n, 3) float32."""
    rs = np.random.RandomState(seed)
    xy = rs.rand(n, 2) * 10.0
    p = np.stack([xy[:, 0], xy[:, 1], 0.3 * xy[:, 0] + 0.1 * xy[:, 1] + 2.0], axis=1)
    return (p + rs.randn(n, 1) * sigma * PLANE_NORMAL).astype(np.float32)

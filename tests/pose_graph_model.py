"""An independent NumPy model of the pose-graph contract (include/icet_hip.h "pose-graph optimisation"), and the loop graphs the tests
share.  Double arithmetic throughout, a dense numpy.linalg.solve per Gauss-Newton iteration, central differences of step 1e-6, the device's accept rule.
Nothing here is shared with the device code: not a header, not the library."""
import numpy as np

JAC_STEP = 1e-6
CONVERGED, ITERATION_CAP, NOT_POSITIVE_DEFINITE, NON_FINITE, STALLED = 0, 1, 2, 3, 4


def wrap(a):
    """Into (-pi, pi]."""
    return -((-a + np.pi) % (2.0 * np.pi) - np.pi)


def xof(Ti, Tj):
    """The predicted measurement of edge (i, j): keyframe i seen from live scan j (the store's START POSE rule, unrounded)."""
    Ri, Rj = Ti[:3, :3], Tj[:3, :3]
    RX = Rj.T @ Ri
    xt = Rj.T @ (Tj[:3, 3] - Ti[:3, 3])
    return np.array([xt[0], xt[1], xt[2], np.arctan2(-RX[2, 1], RX[2, 2]), np.arcsin(np.clip(RX[2, 0], -1.0, 1.0)), np.arctan2(-RX[1, 0], RX[0, 0])])


def exp_se3(d):
    """Exp of delta = (rho, omega) as a 4 x 4 matrix."""
    rho, om = np.asarray(d[:3], np.float64), np.asarray(d[3:], np.float64)
    th = np.linalg.norm(om)
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if th < 1e-5:
        A, B, Cc = 1 - th * th / 6, 0.5 - th * th / 24, 1 / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ rho
    return T


def edge_list(n, closures):
    """(i, j) of every edge: the odometry chain, then the closures."""
    return [(k - 1, k) for k in range(1, n)] + [(int(c[0]), int(c[1])) for c in closures]


def residual(Ti, Tj, X):
    e = xof(Ti, Tj) - np.asarray(X, np.float64)
    e[3:] = wrap(e[3:])
    return e


def edge_chi2(T, edges, X, info):
    out = np.zeros(len(edges))
    for q, (i, j) in enumerate(edges):
        e = residual(T[i], T[j], X[q])
        out[q] = e @ info[q] @ e
    return out


def _measurements(n, odo_X, odo_info, closures):
    X = [np.asarray(x, np.float64) for x in np.asarray(odo_X, np.float32).reshape(-1, 6)] + [np.asarray(c[2], np.float32).astype(np.float64) for c in closures]
    info = [np.asarray(m, np.float32).astype(np.float64).reshape(6, 6) for m in np.asarray(odo_info, np.float32).reshape(-1, 6, 6)] + \
           [np.asarray(c[3], np.float32).astype(np.float64).reshape(6, 6) for c in closures]
    return X, [0.5 * (m + m.T) for m in info]


def jacobians(Ti, Tj):
    J = np.zeros((6, 12))
    for c in range(6):
        d = np.zeros(6); d[c] = JAC_STEP
        Ep, Em = exp_se3(d), exp_se3(-d)
        a = xof(Ti @ Ep, Tj) - xof(Ti @ Em, Tj); a[3:] = wrap(a[3:])
        b = xof(Ti, Tj @ Ep) - xof(Ti, Tj @ Em); b[3:] = wrap(b[3:])
        J[:, c], J[:, 6 + c] = a / (2 * JAC_STEP), b / (2 * JAC_STEP)
    return J


def linearise(T, edges, X, info, is_fixed, damping=0.0):
    """One linearisation at the poses T: (J E x 6 x 12, e E x 6, the dense H and g over the free nodes in ascending order).  H = sum J^T Omega J + damping I."""
    is_fixed = np.asarray(is_fixed, bool)
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(len(is_fixed), int); col[free] = np.arange(free.size)
    m = 6 * free.size
    H, g = np.zeros((m, m)), np.zeros(m)
    Js, es = np.zeros((len(edges), 6, 12)), np.zeros((len(edges), 6))
    for q, (i, j) in enumerate(edges):
        J = jacobians(T[i], T[j])
        e = residual(T[i], T[j], X[q])
        Js[q], es[q] = J, e
        for (a, Ja) in ((i, J[:, :6]), (j, J[:, 6:])):
            if col[a] < 0:
                continue
            sa = slice(6 * col[a], 6 * col[a] + 6)
            g[sa] += Ja.T @ info[q] @ e
            for (b, Jb) in ((i, J[:, :6]), (j, J[:, 6:])):
                if col[b] >= 0:
                    H[sa, 6 * col[b]:6 * col[b] + 6] += Ja.T @ info[q] @ Jb
    H += damping * np.eye(m)
    return Js, es, H, g


def optimise(poses, odo_X, odo_info, closures=(), fixed=None, gn_iters=10, dx_tol=1e-7, damping=0.0):
    """dict(poses float32 N x 4 x 4, poses64, chi2_initial, chi2_final, status, gn_iterations, max_dx, edge_chi2 2 x E)."""
    P32 = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    n = P32.shape[0]
    closures = list(closures)
    edges = edge_list(n, closures)
    X, info = _measurements(n, odo_X, odo_info, closures)
    is_fixed = np.zeros(n, bool); is_fixed[0] = True
    if fixed is not None:
        is_fixed |= np.asarray(fixed).reshape(-1) != 0
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(n, int); col[free] = np.arange(free.size)
    T = P32.astype(np.float64)
    chi0 = edge_chi2(T, edges, X, info)
    chi_e, chi2 = chi0.copy(), float(chi0.sum())
    status, its, max_dx, failed = ITERATION_CAP, 0, 0.0, False
    if not np.isfinite(chi2):
        status, failed = NON_FINITE, True
    for _ in range(gn_iters if not failed else 0):
        its += 1
        m = 6 * free.size
        _, _, H, g = linearise(T, edges, X, info, is_fixed, damping)
        if m:
            if not (np.isfinite(H).all() and np.isfinite(g).all()):
                status, failed = NON_FINITE, True; break
            try:
                np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                status, failed = NOT_POSITIVE_DEFINITE, True; break
            dx = np.linalg.solve(H, -g)
        else:
            dx = np.zeros(0)
        max_dx = float(np.abs(dx).max()) if m else 0.0
        Tt = T.copy()
        for k in free:
            Tt[k] = T[k] @ exp_se3(dx[6 * col[k]:6 * col[k] + 6])
        chit = edge_chi2(Tt, edges, X, info)
        if not np.isfinite(chit.sum()):
            status, failed = NON_FINITE, True; break
        if not (chit.sum() < chi2):
            status = CONVERGED if max_dx < dx_tol else STALLED
            break
        T, chi_e, chi2 = Tt, chit, float(chit.sum())
        if max_dx < dx_tol:
            status = CONVERGED
            break
    out = T.astype(np.float32)
    out[:, 3, :] = (0, 0, 0, 1)
    if failed:
        out, chi_e, chi2 = P32.copy(), chi0, float(chi0.sum())
    out[is_fixed] = P32[is_fixed]
    return dict(poses=out, poses64=T, chi2_initial=float(chi0.sum()), chi2_final=chi2, status=status, gn_iterations=its, max_dx=max_dx, edge_chi2=np.stack([chi0, chi_e]))


# ---- the graphs the tests share: a 30 m loop ----------------------------------------------------------------------------------------------------------------
SIGMA_ODO = (0.01, 0.0005)          # 1 cm, 0.5 mrad per step
SIGMA_CLOSURE = (0.005, 0.0005)     # the smallest sigmas of the test graphs: 5 mm, 0.5 mrad


def diag_info(st, sr):
    return np.diag([1 / st ** 2] * 3 + [1 / sr ** 2] * 3).astype(np.float32)


def _pose_step(X):
    """[R(X)^T | R(X)^T X_t] in double (R = Rx Ry Rz of the library's Euler convention)."""
    ph, th, ps = (float(v) for v in X[3:])
    cph, sph, cth, sth, cps, sps = np.cos(ph), np.sin(ph), np.cos(th), np.sin(th), np.cos(ps), np.sin(ps)
    R = np.array([[cth * cps, sps * cph + sph * sth * cps, sph * sps - sth * cph * cps],
                  [-sps * cth, cph * cps - sph * sth * sps, sph * cps + sth * sps * cph],
                  [sth, -sph * cth, cph * cth]])
    T = np.eye(4); T[:3, :3] = R.T; T[:3, 3] = R.T @ np.asarray(X[:3], np.float64)
    return T


def chain(T0, odo_X):
    """The float32 poses of a chain from T0 and float32 odometry X: T_k = T_(k-1) step(X_k), accumulated in double, rounded once per pose."""
    out = [np.asarray(T0, np.float64)]
    for x in np.asarray(odo_X, np.float32):
        out.append(out[-1] @ _pose_step(x.astype(np.float64)))
    return np.array(out).astype(np.float32)


def make_loop(n, closure_pairs, seed=0, noise=1.0, closure_info=None):
    """A loop of n poses on a 30 m circle with a slow roll and climb.  Odometry X = truth + noise x SIGMA_ODO, the start poses are the chain of that odometry
    (zero odometry residual), closures (i, j) measure the truth + noise x SIGMA_CLOSURE.  Returns dict(truth, poses, odo_X, odo_info, closures)."""
    rng = np.random.default_rng(seed)
    radius = 30.0 / (2 * np.pi)
    truth = []
    for k in range(n):
        a = 2 * np.pi * k / max(n, 2) * (1.0 if n > 3 else 0.2)
        T = exp_se3([0, 0, 0, 0.02 * np.sin(a), 0.03 * np.cos(a), a + np.pi / 2])
        T[:3, 3] = (radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(a))
        truth.append(T)
    truth = np.array(truth)
    so, sc = np.array([SIGMA_ODO[0]] * 3 + [SIGMA_ODO[1]] * 3), np.array([SIGMA_CLOSURE[0]] * 3 + [SIGMA_CLOSURE[1]] * 3)
    odo_X = np.array([xof(truth[k - 1], truth[k]) + noise * so * rng.standard_normal(6) for k in range(1, n)], np.float64).reshape(-1, 6).astype(np.float32)
    odo_info = np.array([diag_info(*SIGMA_ODO)] * (n - 1), np.float32).reshape(-1, 6, 6)
    closures = []
    for q, (i, j) in enumerate(closure_pairs):
        info = diag_info(*SIGMA_CLOSURE) if closure_info is None or closure_info[q] is None else np.asarray(closure_info[q], np.float32)
        closures.append((i, j, (xof(truth[i], truth[j]) + noise * sc * rng.standard_normal(6)).astype(np.float32), info))
    return dict(truth=truth, poses=chain(truth[0].astype(np.float32), odo_X), odo_X=odo_X, odo_info=odo_info, closures=closures)


def pose_error(a, b):
    """(largest translation difference in metres, largest rotation difference in radians) between two pose arrays."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4, 4), np.asarray(b, np.float64).reshape(-1, 4, 4)
    dt = float(np.abs(a[:, :3, 3] - b[:, :3, 3]).max())
    dr = 0.0
    for Ra, Rb in zip(a[:, :3, :3], b[:, :3, :3]):
        D = Ra.T @ Rb
        dr = max(dr, float(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2))
    return dt, dr


# ---- one Gauss-Newton step taken apart (tests/test_pose_graph_step.py) ----------------------------------------------------------------------------------------
def fixed_mask(n, fixed=None):
    m = np.zeros(n, bool); m[0] = True
    if fixed is not None:
        m |= np.asarray(fixed).reshape(-1) != 0
    return m


def dense_from_band(D, B, A, edges, is_fixed, dtype=np.float64):
    """The dense H over the free nodes (ascending) from the device's three arrays: D n x 6 x 6 on the diagonal, B[k] at (k, k - 1) and its transpose at
    (k - 1, k), A[c] at (i, j) of closure c and its transpose at (j, i) where the closure lies off the band between two free nodes.  A fixed node's identity
    block is left out."""
    D, B, A = (np.asarray(v, dtype).reshape(-1, 6, 6) for v in (D, B, A))
    is_fixed = np.asarray(is_fixed, bool)
    n = D.shape[0]
    free = np.nonzero(~is_fixed)[0]
    col = -np.ones(n, int); col[free] = np.arange(free.size)
    H = np.zeros((6 * free.size, 6 * free.size), dtype)

    def blk(a, b):
        return H[6 * col[a]:6 * col[a] + 6, 6 * col[b]:6 * col[b] + 6]
    for k in free:
        blk(k, k)[...] = D[k]
        if k > 0 and col[k - 1] >= 0:
            blk(k, k - 1)[...] = B[k]; blk(k - 1, k)[...] = B[k].T
    for c, (i, j) in enumerate(edges[n - 1:]):
        if abs(i - j) >= 2 and col[i] >= 0 and col[j] >= 0:
            blk(i, j)[...] += A[c]; blk(j, i)[...] += A[c].T
    return H


def band_of(H, is_fixed):
    """The block-tridiagonal part of a dense free-node H: the blocks between nodes whose indices differ by at most one."""
    free = np.nonzero(~np.asarray(is_fixed, bool))[0]
    node = np.repeat(free, 6)
    return np.where(np.abs(node[:, None] - node[None, :]) <= 1, H, 0.0)


def band_solver(M, cholesky=False):
    """r -> M^-1 r.  numpy.linalg.solve is LAPACK's gesv, an LU factorisation with partial pivoting and two triangular solves; with SciPy the same factorisation
    is made once (getrf) and reused (getrs).  `cholesky`: through the Cholesky factor instead -- another float64 solver of the same system."""
    try:
        import scipy.linalg as sl
    except ImportError:
        if cholesky:
            L = np.linalg.cholesky(M)
            return lambda r: np.linalg.solve(L.T, np.linalg.solve(L, r))
        return lambda r: np.linalg.solve(M, r)
    f = sl.cho_factor(M, lower=True) if cholesky else sl.lu_factor(M)
    return (lambda r: sl.cho_solve(f, r)) if cholesky else (lambda r: sl.lu_solve(f, r))


def precond_ratio(H, g, M, x):
    """sqrt(r . M^-1 r / g . M^-1 g) of the TRUE residual r = -g - H x."""
    r = -g - H @ x
    return float(np.sqrt((r @ np.linalg.solve(M, r)) / (g @ np.linalg.solve(M, g))))


def pcg_reference(H, g, band_of_H, tol, cap):
    """Textbook preconditioned conjugate gradients on H x = -g in float64, the dense band through numpy.linalg.solve as preconditioner, with the driver's stop
    rule: per iteration a band solve and r.z, the end at r.z == 0 or (from the second iteration) sqrt(r.z / r0.z0) <= tol, else a step; at most `cap` band
    solves.  dict(x, iterations (the steps taken: exact arithmetic needs at most rank(H - M) + 1), band_solves (one more where the end was found by a band solve
    behind the last step), ratio (precond_ratio of x), end ("tolerance" | "zero" | "cap"), rz, pq)."""
    x, r = np.zeros_like(g), -g.copy()
    p, rz_prev, rz0, its, end, rzs, pqs = None, None, None, 0, "cap", [], []
    solve = band_solver(band_of_H)
    for ci in range(cap):
        z = solve(r)
        rz = float(r @ z)
        its += 1; rzs.append(rz)
        if ci == 0:
            rz0, p = rz, z
        else:
            p = z + (rz / rz_prev) * p
        if rz == 0.0:
            end = "zero"; break
        if ci > 0 and np.sqrt(rz / rz0) <= tol:
            end = "tolerance"; break
        q = H @ p
        pq = float(p @ q); pqs.append(pq)
        alpha = rz / pq
        x, r, rz_prev = x + alpha * p, r - alpha * q, rz
    return dict(x=x, iterations=len(pqs), band_solves=its, ratio=precond_ratio(H, g, band_of_H, x), end=end, rz=rzs, pq=pqs)


# the Jacobians once more in numpy.longdouble: the same central differences of the same step from the same float64 poses.  Only to measure how far the float64
# evaluation is from itself at higher precision (its rounding noise, about eps |xof| / 2 h).
_LD = np.longdouble
_PI_LD = 4 * np.arctan(_LD(1))


def _wrap_ld(a):
    return -((-a + _PI_LD) % (2 * _PI_LD) - _PI_LD)


def xof_ld(Ti, Tj):
    Ti, Tj = np.asarray(Ti, _LD), np.asarray(Tj, _LD)
    RX = Tj[:3, :3].T @ Ti[:3, :3]
    xt = Tj[:3, :3].T @ (Tj[:3, 3] - Ti[:3, 3])
    return np.array([xt[0], xt[1], xt[2], np.arctan2(-RX[2, 1], RX[2, 2]), np.arcsin(np.clip(RX[2, 0], _LD(-1), _LD(1))), np.arctan2(-RX[1, 0], RX[0, 0])], _LD)


def exp_se3_ld(d):
    d = np.asarray(d, _LD)
    rho, om = d[:3], d[3:]
    th = np.sqrt(om @ om)
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]], _LD)
    if th < 1e-5:
        A, B, Cc = 1 - th * th / 6, _LD(0.5) - th * th / 24, _LD(1) / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4, dtype=_LD)
    T[:3, :3] = np.eye(3, dtype=_LD) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3, dtype=_LD) + B * K + Cc * (K @ K)) @ rho
    return T


def jacobians_ld(Ti, Tj):
    Ti, Tj = np.asarray(Ti, _LD), np.asarray(Tj, _LD)
    h = _LD(JAC_STEP)
    J = np.zeros((6, 12), _LD)
    for c in range(6):
        d = np.zeros(6, _LD); d[c] = h
        Ep, Em = exp_se3_ld(d), exp_se3_ld(-d)
        a = xof_ld(Ti @ Ep, Tj) - xof_ld(Ti @ Em, Tj); a[3:] = _wrap_ld(a[3:])
        b = xof_ld(Ti, Tj @ Ep) - xof_ld(Ti, Tj @ Em); b[3:] = _wrap_ld(b[3:])
        J[:, c], J[:, 6 + c] = a / (2 * h), b / (2 * h)
    return J

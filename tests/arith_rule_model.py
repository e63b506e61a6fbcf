"""A model of THE SHARED ARITHMETIC RULE for cartesianToSpherical / sphericalToCartesian -- the stated rule, not the device's formulas.

    r      plain IEEE float32: x*x + y*y, then + z*z, then sqrt (src/utils.cpp:99); NaN -> 1000 afterwards
    theta  the correctly rounded float32 of the exact atan2(y, x); a negative one is wrapped as (float)((double)t + 2 pi_double); NaN -> 1000
    phi    the correctly rounded float32 of the exact acos(q), q = z / r the float32 quotient (r before its sentinel); NaN -> 1000
    out    (r sin phi cos theta, r sin phi sin theta, r cos phi), the four sines / cosines correctly rounded from the float32 angles, the
           products left to right in float32 (src/utils.cpp:134-136)

"Correctly rounded" is decided by mpmath at PREC bits.  The vectorised path evaluates the function in float64 (an error of about 2^-52 relative) and rounds that;
every value whose float64 result lies within GUARD = 2^-40 relative of a float32 rounding boundary is decided again from the exact value, so the float64 library
never decides a close call.  algebraic_roundtrip() restates, in IEEE float64 without contraction, the algebraic form the device evaluates on its common path
(icet_device_common.h roundtrip_cr without its small-value branch): tests use it to show that their inputs can tell the two apart.
"""
import numpy as np
import mpmath

F32, F64 = np.float32, np.float64
PREC = 256
GUARD = 2.0 ** -40
TWO_PI = 2.0 * np.pi                        # the reference's double constant 2 * M_PI
TWO_PI_TAIL = 2.4492935982947064e-16        # (exact 2 pi) - TWO_PI


def _mpf(v):
    return mpmath.mpf(float(v))


def f32_neighbours(f):
    """The two rounding boundaries (float64, exact) around the float32 values f: midpoints to the next float32 below and above."""
    f = np.asarray(f, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = (np.nextafter(f, F32(-np.inf)).astype(F64) + f.astype(F64)) * 0.5
        hi = (np.nextafter(f, F32(np.inf)).astype(F64) + f.astype(F64)) * 0.5
    return lo, hi


def round_exact_to_f32(xm):
    """The float32 nearest to the mpf xm, ties to even (subnormals included).  xm is not zero."""
    f0 = F32(float(xm))
    cands = (np.nextafter(f0, F32(-np.inf)), f0, np.nextafter(f0, F32(np.inf)))
    return min(cands, key=lambda c: (abs(xm - _mpf(c)), int(np.asarray(c).view(np.uint32)) & 1))


def boundary_distance(xm):
    """Absolute distance (float) of the exact value xm to the nearest float32 rounding boundary."""
    f = np.asarray(round_exact_to_f32(xm), F32).reshape(1)
    lo, hi = f32_neighbours(f)
    return float(min(abs(xm - _mpf(lo[0])), abs(_mpf(hi[0]) - xm)))


def cr_round(v64, exact, stats=None):
    """float64 evaluations v64 -> correctly rounded float32; exact(i) returns element i's exact value as an mpf (called inside workprec(PREC))."""
    v64 = np.asarray(v64, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v64.astype(F32)
        lo, hi = f32_neighbours(f)
        dist = np.minimum(np.abs(v64 - lo), np.abs(hi - v64))
        sus = np.isfinite(v64) & (v64 != 0.0) & (dist <= GUARD * np.abs(v64))
    idx = np.flatnonzero(sus)
    if idx.size:
        with mpmath.workprec(PREC):
            for i in idx:
                f[i] = round_exact_to_f32(exact(int(i)))
    if stats is not None:
        stats["redecided"] = stats.get("redecided", 0) + int(idx.size)
    return f


def exact_atan2(y, x):
    a = mpmath.atan2(abs(_mpf(y)), _mpf(x))
    return -a if np.signbit(y) else a


def radius_raw(x, y, z):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = x * x + y * y
        s = s + z * z
        return np.sqrt(s)


def atan2_cr(y, x, stats=None):
    yd, xd = np.asarray(y, F32).astype(F64), np.asarray(x, F32).astype(F64)
    return cr_round(np.arctan2(yd, xd), lambda i: exact_atan2(yd[i], xd[i]), stats)


def acos_cr(q, stats=None):
    qd = np.asarray(q, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        return cr_round(np.arccos(qd), lambda i: mpmath.acos(_mpf(qd[i])), stats)


def sin_cr(a, stats=None):
    ad = np.asarray(a, F32).astype(F64)
    return cr_round(np.sin(ad), lambda i: mpmath.sin(_mpf(ad[i])), stats)


def cos_cr(a, stats=None):
    ad = np.asarray(a, F32).astype(F64)
    return cr_round(np.cos(ad), lambda i: mpmath.cos(_mpf(ad[i])), stats)


def c2s(xyz, stats=None):
    """(N, 3) float32 r | theta | phi with the reference's NaN -> 1000 sentinels, and r before its sentinel."""
    p = np.asarray(xyz, F32)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    rr = radius_raw(x, y, z)
    th = atan2_cr(y, x, stats)
    neg = th < 0                                           # (-0 is not negative: it stays)
    with np.errstate(invalid="ignore"):
        th = np.where(neg, (th.astype(F64) + TWO_PI).astype(F32), th)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = z / rr
    ph = acos_cr(q, stats)
    s = lambda a: np.where(np.isnan(a), F32(1000.0), a).astype(F32)
    return np.stack([s(rr), s(th), s(ph)], 1), rr


def voxel_of(sph, T, P):
    bt = ((sph[:, 1].astype(F64) / TWO_PI) * T).astype(np.int64) % T
    bp = ((sph[:, 2].astype(F64) / np.pi) * P).astype(np.int64) % P
    return (T * bp + bt).astype(np.int32)


def s2c(sph, stats=None):
    r, th, ph = sph[:, 0], sph[:, 1], sph[:, 2]
    sp, cp, st, ct = sin_cr(ph, stats), cos_cr(ph, stats), sin_cr(th, stats), cos_cr(th, stats)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.stack([(r * sp) * ct, (r * sp) * st, r * cp], 1).astype(F32)


def model(xyz, T=75, P=24):
    """Everything icet_debug_spherical returns, from the rule: dict(sph, voxel, rt, ordinary, redecided).  ordinary: rows with a finite r > 0, the ones the direct
    roundtrip_cr serves (for them its theta | phi | x | y | z are sph[:, 1:] and rt)."""
    stats = {}
    sph, rr = c2s(xyz, stats)
    with np.errstate(invalid="ignore"):
        ordinary = (rr > 0) & (rr < np.inf)
    return dict(sph=sph, voxel=voxel_of(sph, T, P), rt=s2c(sph, stats), ordinary=ordinary, redecided=stats.get("redecided", 0))


def algebraic_roundtrip(xyz):
    """The device's common-path evaluation (roundtrip_cr's algebraic sines / cosines, no small-value branch) restated in IEEE float64 for rows with a finite r > 0:
    sin a_f = sin a_d (1 - d^2/2) + cos a_d d with a_d the float64 angle, d = a_f - a_d, sin a_d and cos a_d algebraic in the inputs.  (N, 3) float32; other rows NaN."""
    p = np.asarray(xyz, F32)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    rr = radius_raw(x, y, z)
    with np.errstate(all="ignore"):
        ok = (rr > 0) & (rr < np.inf)
        xd, yd = x.astype(F64), y.astype(F64)
        td = np.arctan2(yd, xd)
        t0 = td.astype(F32)
        wrap = t0 < 0
        th = np.where(wrap, (t0.astype(F64) + TWO_PI).astype(F32), t0)
        dth = np.where(wrap, ((th.astype(F64) - TWO_PI) - td) - TWO_PI_TAIL, th.astype(F64) - td)
        rho2 = xd * xd + yd * yd
        inv = 1.0 / np.sqrt(rho2)
        s0 = np.where(rho2 > 0, yd * inv, 0.0)
        c0 = np.where(rho2 > 0, xd * inv, np.where(np.signbit(x), -1.0, 1.0))
        hth = 0.5 * dth * dth
        st = s0 + (c0 * dth - s0 * hth)
        ct = c0 - (s0 * dth + c0 * hth)
        qd = (z / rr).astype(F64)
        pd = np.arccos(qd)
        ph = pd.astype(F32)
        dph = ph.astype(F64) - pd
        sp0 = np.sqrt((1.0 - qd) * (1.0 + qd))
        hph = 0.5 * dph * dph
        sp = sp0 + (qd * dph - sp0 * hph)
        cp = qd - (sp0 * dph + qd * hph)
        stf, ctf, spf, cpf = st.astype(F32), ct.astype(F32), sp.astype(F32), cp.astype(F32)
        out = np.stack([(rr * spf) * ctf, (rr * spf) * stf, rr * cpf], 1).astype(F32)
    out[~ok] = np.nan
    return out


def same_bits(a, b):
    """Row mask: float32 arrays a, b equal bit for bit (sign of zero included; a NaN equals any NaN)."""
    a = np.asarray(a, F32).reshape(len(a), -1); b = np.asarray(b, F32).reshape(len(b), -1)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(1)

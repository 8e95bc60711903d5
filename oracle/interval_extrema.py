"""Python mirror of the kernel's grid-extrema candidate rule -- TEST INFRASTRUCTURE,
NOT PRODUCT CODE.

``interval_extrema_on`` (sacenv_boat_wind.h) finds the extreme grid samples of one spline
interval among ten candidates: the interval's first and last grid index and the four
neighbours of each critical point. This is that rule in float64 Python (exact ``sqrt``
and division where the kernel uses approximations), returning the candidate indices.
tests/test_host_cpu.py proves it on random curves, tests/test_wind_fit_mp_cpu.py on
the adversarial ones of oracle/wind_fit_cases.py.
"""
import math


def interval_extrema_py(y, m, n, L, j):
    """Python mirror of the kernel's interval_extrema candidate rule -> grid indices."""
    step = (n - 1) / (L - 1)
    jf = lambda i: min(int(i * step), n - 2)

    inv = (L - 1) / (n - 1)        # the host's knot_inv (sacenv/config.py)
    lo = max(math.ceil(j * inv) - 1, 0)
    while lo < L and jf(lo) < j:
        lo += 1
    hi = min(math.floor((j + 1) * inv) + 1, L - 1)
    while hi >= 0 and jf(hi) > j:
        hi -= 1
    if lo > hi:
        return [], []
    cand = [lo, hi]
    a, b = m[j], m[j + 1]
    qa, qb, qc = 3 * (b - a), 6 * a, y[j + 1] - y[j] - 2 * a - b
    roots = []
    scale = abs(qa) + abs(qb) + abs(qc)
    if abs(qa) <= 1e-14 * scale:
        if qb != 0:
            roots.append(-qc / qb)
    else:
        if scale < 2.0 ** -500:            # a tiny curve: scaled into [0.5, 1), its squares do not underflow
            up = -math.frexp(scale)[1]     # (ldexp per coefficient: exact down to subnormal knots)
            qa, qb, qc = math.ldexp(qa, up), math.ldexp(qb, up), math.ldexp(qc, up)
        disc = qb * qb - 4 * qa * qc
        if disc >= 0:
            q = -0.5 * (qb + math.copysign(math.sqrt(disc), qb if qb != 0 else 1.0))
            roots.append(q / qa)
            if q != 0:
                roots.append(qc / q)
    for tr in roots:
        if not (-0.01 < tr < 1.01):
            continue
        i0 = math.floor((j + tr) * inv)
        for d in (-1, 0, 1, 2):
            cand.append(min(max(i0 + d, lo), hi))
    return cand, (lo, hi)

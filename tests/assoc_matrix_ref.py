"""Reference for vs_query_assoc_matrix in numpy and Python integers: the quantiser (frexp, rint on float64), the balanced limb split,
S = D @ q in int64 and the CHI2 cell from exact integers with float() conversions (Python rounds an int to the nearest double, ties to
even, which is what the engine's conversions do)."""
import numpy as np

LIMBS = 4


def shifts(y):
    """f_k = 30 - e with max |y_k| = m 2^e, 0.5 <= m < 1; 0 for a column of zeros."""
    y = np.asarray(y, np.float32)
    m = np.abs(y.astype(np.float64)).max(axis=0)
    _, e = np.frexp(m)
    return np.where(m == 0, 0, 30 - e).astype(np.int32)


def quantise(y):
    """(q int64 (n, K), shift int32 (K,)): q = rint(y 2^f) on float64, ties to even."""
    y = np.asarray(y, np.float32)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    f = shifts(y)
    q = np.rint(np.ldexp(y.astype(np.float64), f[None, :])).astype(np.int64)
    assert (np.abs(q) < 2 ** 30).all()
    return q, f


def limbs(q):
    """The four balanced base-256 digits of every q, low to high: (..., 4) int64, each in [-128, 127]."""
    q = np.asarray(q, np.int64).copy()
    out = np.zeros(q.shape + (LIMBS,), np.int64)
    for l in range(LIMBS):
        b = ((q + 128) & 255) - 128
        out[..., l] = b
        q = (q - b) >> 8
    assert not q.any()
    return out


def dot(dosage, q):
    """S = D @ q in int64: dosage (A, n) of 0 / 1 / 2, q (n, K)."""
    return np.asarray(dosage, np.int64) @ np.asarray(q, np.int64)


def dot_by_limbs(dosage, q):
    """The same through the four limb sums, as the kernel forms it."""
    d = np.asarray(dosage, np.int64)
    b = limbs(q)
    acc = [d @ b[..., l] for l in range(LIMBS)]
    assert all(np.abs(a).max(initial=0) < 2 ** 31 for a in acc)
    return acc[0] + (acc[1] << 8) + (acc[2] << 16) + (acc[3] << 24)


def scores_dot(S, f):
    return np.ldexp(S.astype(np.float64), -np.asarray(f, np.int32)[None, :])


def trait_moments(q):
    """(Sy, Syy, vy) per trait as Python integers."""
    n = q.shape[0]
    sy = [sum(int(v) for v in q[:, k]) for k in range(q.shape[1])]
    syy = [sum(int(v) * int(v) for v in q[:, k]) for k in range(q.shape[1])]
    return sy, syy, [n * b - a * a for a, b in zip(sy, syy)]


def chi2(n, ac, hom, S, q):
    """The score test from exact integers: ac / hom the rows' alt_alleles and hom_alt over the columns."""
    sy, _syy, vy = trait_moments(q)
    out = np.zeros(S.shape, np.float64)
    for i in range(S.shape[0]):
        sx = int(ac[i])
        vx = n * (sx + 2 * int(hom[i])) - sx * sx
        for k in range(S.shape[1]):
            if vx == 0 or vy[k] <= 0:
                continue
            cov = float(n * int(S[i, k]) - sx * sy[k])
            out[i, k] = ((float(n) * cov) * cov) / (float(vx) * float(vy[k]))
    return out


def trait_sums(q, f):
    """trait_sum / trait_sumsq as the result carries them."""
    sy, syy, _ = trait_moments(q)
    return (np.array([np.ldexp(float(a), -int(s)) for a, s in zip(sy, f)]),
            np.array([np.ldexp(float(b), -2 * int(s)) for b, s in zip(syy, f)]))


# q values whose limbs sit at both extremes and that exercise the carries between limbs
# (every one fits float32's 24 bits, so ldexp builds a trait value that quantises back to it)
CHOSEN_Q = [0, 1, -1, 127, 128, 129, 255, 256, -128, -129, 0x7F7F7F, 0x808080, -0x808080, 0x7F7F7F << 6, 127 << 8, -(128 << 8),
            127 << 16, -(128 << 16), 2 ** 30 - 64, -(2 ** 30 - 64)]


def chosen_traits(n, rng=None):
    """An (n, 2) float32 panel built by ldexp from chosen q: column 0 cycles through CHOSEN_Q with the largest first (so the shift
    is 0 and q comes back as chosen), column 1 the same scaled by 2^-20 and reversed."""
    base = [2 ** 30 - 64] + CHOSEN_Q
    c0 = np.array([base[i % len(base)] for i in range(n)], np.int64)
    c1 = c0[::-1].copy()
    c1[0] = 2 ** 30 - 64
    y = np.stack([c0.astype(np.float64), np.ldexp(c1.astype(np.float64), -20)], axis=1)
    return y.astype(np.float32), np.stack([c0, c1], axis=1)


def chi2_table(n, ac, hom, S, q):
    """chi2() for a whole table at once: the same integers through int64 where they fit (asserted), vy through Python integers, the
    same float conversions (numpy's cast of an int64 rounds to nearest, ties to even, as float() does)."""
    sy, _syy, vy = trait_moments(q)
    S = np.asarray(S, np.int64)
    sx = np.asarray(ac, np.int64)
    vx = n * (sx + 2 * np.asarray(hom, np.int64)) - sx * sx
    assert n * int(np.abs(S).max(initial=0)) < 2 ** 62 and int(sx.max(initial=0)) * max([abs(v) for v in sy] + [0]) < 2 ** 62
    cov = (n * S - sx[:, None] * np.array(sy, np.int64)[None, :]).astype(np.float64)
    vyf = np.array([float(v) for v in vy])
    ok = (vx != 0)[:, None] & (np.array([v > 0 for v in vy]))[None, :]
    den = np.where(ok, vx.astype(np.float64)[:, None] * vyf[None, :], 1.0)
    return np.where(ok, ((float(n) * cov) * cov) / den, 0.0)

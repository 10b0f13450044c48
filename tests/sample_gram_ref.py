"""The expected answer of a sample Gram query (vs_query_sample_gram), worked out from a genotype matrix: the uint8 cells that
genotype_matrix_ref.matrix derives from the oracle's type-6 text, or any matrix of such cells (rows x columns).  The sums are int64;
the GRM's numerator is formed with Python integers, each of the two conversions to float64 rounds once, one division follows -- as
the interface defines it."""
import numpy as np

from ld_band_ref import dosage


def sample_gram(m):
    """(gram, s, C, H) of a rows x n matrix of cells: gram = D^T D (int64, (n, n)), ac = the row sums of the dosages (a row's
    alt_alleles over the columns), s = D^T ac (int64, (n,)), C = sum ac^2 and H = sum ac (2 n - ac) (Python ints)."""
    d = dosage(m)
    n = d.shape[1]
    ac = d.sum(axis=1)
    gram = d.T @ d
    s = d.T @ ac
    return gram, s, int((ac * ac).sum()), int((ac * (2 * n - ac)).sum())


def grm_numerator(gram, s, c):
    """num_ij = n^2 G_ij - n (s_i + s_j) + C as Python integers (dtype=object, (n, n))."""
    n = int(gram.shape[0])
    g = np.asarray(gram).astype(object)
    so = np.asarray(s).astype(object)
    return g * (n * n) - (so[:, None] + so[None, :]) * n + int(c)


def grm(gram, s, c, h):
    """float64 (n, n): float(2 num_ij) / float(H), and 0.0 where H == 0.  Also returns num."""
    num = grm_numerator(gram, s, c)
    n = num.shape[0]
    if h == 0:
        return np.zeros((n, n), np.float64), num
    top = np.asarray([float(2 * int(x)) for x in num.ravel()], np.float64).reshape(n, n)   # (int -> float rounds to nearest even)
    return top / float(int(h)), num


def gram_text(names, values, stat):
    """What `variantstore gram` writes: a header line of the sample names, then a line per sample: its name and its row, the
    values as %lld ("dot") or %.17g ("grm")."""
    out = "Sample" + "".join("\t" + nm for nm in names) + "\n"
    for i, nm in enumerate(names):
        out += nm + "".join("\t" + (("%d" % int(v)) if stat == "dot" else ("%.17g" % float(v))) for v in values[i]) + "\n"
    return out

"""The expected answer of a burden query (vs_query_sample_burden), worked out from query type 6's text (print_var: `name(g1 sep
g2) ` per carrier, the index's genotype bits) -- the oracle has no burden function of its own."""
import re

import numpy as np

HEADER = "Sample\tVariants\tAC\tHomAlt\tPhased\n"
FIELDS = ("variants", "alt_alleles", "hom_alt", "phased")
NO_MAX = 0xFFFFFFFF


_CARRIER = re.compile(r"([^ \t]+)\(([01])([|/])([01])\) ")


class Parsed:
    """The carriers of a batch's type-6 texts as flat arrays (one pass over the text, shared by every subset and window that is
    checked against it): per carrier its region, its row (numbered over the whole batch), its name's number and genotype bits."""

    def __init__(self, texts):
        self.n_regions = len(texts)
        self.name_no = {}
        q_of, row_of, name_of, g1, g2, ph = [], [], [], [], [], []
        n_rows = 0
        for q, text in enumerate(texts):
            if text is None:
                continue
            for line in text.split("\n")[1:]:
                if not line:
                    continue
                for name, a, sep, b in _CARRIER.findall(line.split("\t", 3)[3]):
                    q_of.append(q); row_of.append(n_rows)
                    name_of.append(self.name_no.setdefault(name, len(self.name_no)))
                    g1.append(a == "1"); g2.append(b == "1"); ph.append(sep == "|")
                n_rows += 1
        self.n_rows = n_rows
        self.q_of, self.row_of, self.name_of = (np.asarray(v, np.int64) for v in (q_of, row_of, name_of))
        self.g1, self.g2, self.ph = (np.asarray(v, np.int64) for v in (g1, g2, ph))


def burden_sparse(texts, columns_by_name, min_ac=0, max_ac=NO_MAX):
    """The nonzero cells of burden_matrix: (flat cell numbers q * C + c, ascending; int64 (n, 4) values)."""
    p = texts if isinstance(texts, Parsed) else Parsed(texts)
    col_of = np.full(len(p.name_no) + 1, -1, np.int64)
    for c, name in enumerate(columns_by_name):
        if name in p.name_no:
            col_of[p.name_no[name]] = c
    col = col_of[p.name_of]
    sel = col >= 0
    alt = p.g1 + p.g2
    ac_row = np.bincount(p.row_of[sel], weights=alt[sel], minlength=p.n_rows + 1).astype(np.int64)   # over the columns' samples alone
    ok = sel & (ac_row[p.row_of] >= min_ac) & (ac_row[p.row_of] <= max_ac)
    flat = p.q_of[ok] * len(columns_by_name) + col[ok]
    cells, inv = np.unique(flat, return_inverse=True)
    vals = np.stack([np.bincount(inv, weights=w, minlength=cells.shape[0]).astype(np.int64)
                     for w in (np.ones(inv.shape[0]), alt[ok], (p.g1 & p.g2)[ok], p.ph[ok])], axis=-1).reshape(-1, 4)
    return cells, vals


def burden_matrix(texts, columns_by_name, min_ac=0, max_ac=NO_MAX):
    """int64 (Q, C, 4) -- variants, alt_alleles, hom_alt, phased per (region, column) -- from the type-6 texts of the regions
    (None: a region to be skipped, its row stays 0; or a Parsed batch).  `columns_by_name`: the column names in column order;
    they are also the sample set S over which a row's alternate-allele count is taken for the window [min_ac, max_ac]."""
    n = texts.n_regions if isinstance(texts, Parsed) else len(texts)
    cells, vals = burden_sparse(texts, columns_by_name, min_ac, max_ac)
    out = np.zeros((n * len(columns_by_name), 4), np.int64)
    out[cells] = vals
    return out.reshape(n, len(columns_by_name), 4)


def burden_text(cells_q, columns_by_name):
    """The text vs_result_format_region gives for a burden region, from its row of burden_matrix."""
    return HEADER + "".join(f"{name}\t" + "\t".join(str(int(v)) for v in cells_q[c]) + "\n"
                            for c, name in enumerate(columns_by_name) if cells_q[c][0] > 0)


def cells_array(cells):
    """A structured (Q, C) cell array of QueryResult.sample_burden as int64 (Q, C, 4)."""
    return np.stack([cells[f].astype(np.int64) for f in FIELDS], axis=-1)

"""The expected answer of a genotype-matrix query (vs_query_genotype_matrix), worked out from query type 6's text (print_var:
`name(g1 sep g2) ` per carrier, the index's genotype bits) -- the oracle has no matrix function of its own.  The rows are the
rows the texts list, region after region: what a result reports for region q without the rows the duplicate rule dropped."""
import re

import numpy as np

_CARRIER = re.compile(r"([^ \t]+)\(([01])([|/])([01])\) ")


def cell(g1, g2, phased):
    """The byte of a carrier: 0x08 | phase | gt_1 << 1 | gt_2 << 2."""
    return 0x08 | int(bool(phased)) | (int(bool(g1)) << 1) | (int(bool(g2)) << 2)


class Parsed:
    """The rows and carriers of a batch's type-6 texts (None: a region to be skipped, it has no rows), parsed once and shared by
    every sample set that is checked against it.  row_begin[q], row_count[q]: region q's rows among all n_rows; heads[i]: the
    `Pos\\tRef\\tAlt` of row i as the text has it; per carrier its row, its name's number and its byte."""

    def __init__(self, texts):
        self.n_regions = len(texts)
        self.name_no = {}
        self.heads = []
        self.row_begin = np.zeros(len(texts), np.int64)
        self.row_count = np.zeros(len(texts), np.int64)
        row_of, name_of, val = [], [], []
        for q, text in enumerate(texts):
            self.row_begin[q] = len(self.heads)
            if text is None:
                continue
            for line in text.split("\n")[1:]:
                if not line:
                    continue
                pos, ref, alt, carriers = line.split("\t", 3)
                for name, a, sep, b in _CARRIER.findall(carriers):
                    row_of.append(len(self.heads))
                    name_of.append(self.name_no.setdefault(name, len(self.name_no)))
                    val.append(cell(a == "1", b == "1", sep == "|"))
                self.heads.append(f"{pos}\t{ref}\t{alt}")
            self.row_count[q] = len(self.heads) - self.row_begin[q]
        self.n_rows = len(self.heads)
        self.row_of, self.name_of = np.asarray(row_of, np.int64), np.asarray(name_of, np.int64)
        self.val = np.asarray(val, np.uint8)


def matrix_sparse(texts, columns_by_name):
    """The nonzero cells: (row, column, byte) arrays, rows numbered as in Parsed, sorted by (row, column)."""
    p = texts if isinstance(texts, Parsed) else Parsed(texts)
    col_of = np.full(len(p.name_no) + 1, -1, np.int64)
    for c, name in enumerate(columns_by_name):
        if name in p.name_no:
            col_of[p.name_no[name]] = c
    col = col_of[p.name_of] if p.name_of.size else np.zeros(0, np.int64)
    sel = col >= 0
    row, col, val = p.row_of[sel], col[sel], p.val[sel]
    order = np.lexsort((col, row))
    return row[order], col[order], val[order]


def matrix(texts, columns_by_name):
    """uint8 (n_rows, C): the expected matrix over the rows of Parsed, `columns_by_name` the column names in column order."""
    p = texts if isinstance(texts, Parsed) else Parsed(texts)
    row, col, val = matrix_sparse(p, columns_by_name)
    out = np.zeros((p.n_rows, len(columns_by_name)), np.uint8)
    out[row, col] = val
    return out


def call_text(v):
    """A cell as vs_result_format_region writes it: `0`, or gt_1, the separator of print_var, gt_2."""
    v = int(v)
    return "0" if v == 0 else f"{(v >> 1) & 1}{'|' if v & 1 else '/'}{(v >> 2) & 1}"


def matrix_text(parsed, q, m, columns_by_name):
    """The text vs_result_format_region gives for region q of a matrix result: m is matrix(parsed, columns_by_name)."""
    head = "Pos\tRef\tAlt" + "".join("\t" + n for n in columns_by_name) + "\n"
    a0 = int(parsed.row_begin[q])
    return head + "".join(parsed.heads[i] + "".join("\t" + call_text(v) for v in m[i]) + "\n"
                          for i in range(a0, a0 + int(parsed.row_count[q])))

"""The expected answer of a grouped-count query, worked out from query type 6's text and a {sample name -> group index} map:
allele_counts_ref.count_rows once per group -- the oracle has no count function of its own."""
import numpy as np

from allele_counts_ref import count_rows

HEADER = "Pos\tRef\tAlt\tGroup\tN\tCarriers\tAC\tHomAlt\tPhased\n"


def group_members(group_of, n_groups):
    """[set of sample names] per group from {name: group index}; samples that are not in the map belong to no group."""
    members = [set() for _ in range(n_groups)]
    for name, g in group_of.items():
        members[g].add(name)
    return members


def group_rows(text, group_of, n_groups):
    """[(pos, ref, alt, [(carriers, alt_alleles, hom_alt, phased) per group])] of a type-6 region text."""
    per_group = [count_rows(text, m) for m in group_members(group_of, n_groups)]
    return [(row[0], row[1], row[2], [tuple(per_group[g][i][3:]) for g in range(n_groups)]) for i, row in enumerate(per_group[0])]


def groups_text(text, group_of, n_groups, names=None):
    """The text vs_result_format_region gives for a grouped-count region, from the type-6 text of the same region; `names`: the
    groups' names (None: their decimal indices)."""
    sizes = [len(m) for m in group_members(group_of, n_groups)]
    out = [HEADER]
    for pos, ref, alt, counts in group_rows(text, group_of, n_groups):
        for g in range(n_groups):
            label = str(g) if names is None else names[g]
            out.append("\t".join([str(pos), ref, alt, label, str(sizes[g])] + [str(v) for v in counts[g]]) + "\n")
    return "".join(out)


# ---- the same in one pass over a region's carriers, for cohorts too large for a count_rows call per group -------------------
def parse_region(text, ids_of):
    """A type-6 region text as arrays: ([`pos\\tref\\talt\\t` per row], and per carrier: sample id (ids_of: name -> id), its row,
    gt_1 + gt_2, gt_1 and gt_2, the phase bit)."""
    heads, ids, row_of, ac, hom, ph = [], [], [], [], [], []
    for line in text.split("\n")[1:]:
        if not line:
            continue
        pos, ref, alt, samples = line.split("\t")
        i = len(heads)
        heads.append(f"{pos}\t{ref}\t{alt}\t")
        for tok in samples.split(" "):
            if not tok:
                continue
            name, gt = tok[:-1].rsplit("(", 1)
            g1, g2 = gt[0] == "1", gt[2] == "1"
            ids.append(ids_of[name]); row_of.append(i); ac.append(int(g1) + int(g2)); hom.append(int(g1 and g2)); ph.append(int(gt[1] == "|"))
    return heads, np.array(ids, np.int64), np.array(row_of, np.int64), np.array(ac, np.int64), np.array(hom, np.int64), np.array(ph, np.int64)


def parsed_groups_text(parsed, label, n_groups, names=None):
    """groups_text from parse_region's arrays; `label`: integer array over the sample ids, the group of each or -1."""
    heads, ids, row_of, ac, hom, ph = parsed
    sizes = np.bincount(label[label >= 0], minlength=n_groups)
    lab = label[ids] if ids.shape[0] else ids
    keep = lab >= 0
    key = row_of[keep] * n_groups + lab[keep]
    cells = len(heads) * n_groups
    fields = [np.bincount(key, minlength=cells)] + [np.bincount(key, weights=w[keep], minlength=cells).astype(np.int64) for w in (ac, hom, ph)]
    out = [HEADER]
    for i, head in enumerate(heads):
        for g in range(n_groups):
            c = i * n_groups + g
            out.append(f"{head}{g if names is None else names[g]}\t{sizes[g]}\t{fields[0][c]}\t{fields[1][c]}\t{fields[2][c]}\t{fields[3][c]}\n")
    return "".join(out)

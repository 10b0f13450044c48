"""The expected answer of an allele-count query, worked out from query type 6's text (print_var: `name(g1 sep g2) ` per
carrier, the index's genotype bits) -- the oracle has no count function of its own."""

HEADER = "Pos\tRef\tAlt\tCarriers\tAC\tHomAlt\tPhased\n"


def count_rows(text, subset=None):
    """[(pos, ref, alt, carriers, alt_alleles, hom_alt, phased)] of a type-6 region text, over the carriers whose names are in
    `subset` (None: every carrier).  gt_1 / gt_2 are the characters around the separator, '|' marks a phased call."""
    out = []
    for line in text.split("\n")[1:]:
        if not line:
            continue
        pos, ref, alt, samples = line.split("\t")
        car = ac = hom = ph = 0
        for tok in samples.split(" "):
            if not tok:
                continue
            name, gt = tok[:-1].rsplit("(", 1)
            if subset is not None and name not in subset:
                continue
            g1, g2 = gt[0] == "1", gt[2] == "1"
            car += 1
            ac += int(g1) + int(g2)
            hom += int(g1 and g2)
            ph += int(gt[1] == "|")
        out.append((int(pos), ref, alt, car, ac, hom, ph))
    return out


def counts_text(text, subset=None):
    """The text vs_result_format_region gives for an allele-count region, from the type-6 text of the same region."""
    return HEADER + "".join("\t".join(str(v) for v in row) + "\n" for row in count_rows(text, subset))

"""Test helpers: random FASTA/VCF cohorts and oracle comparison."""
import os

import numpy as np

BASES = "ACGT"


def write_random_cohort(dirpath, seed, ref_len=4000, n_rows=120, n_samples=6, sample_names=None,
                        p_ins=0.12, p_del=0.12, p_multi=0.08, p_mnp=0.05, p_near=0.3, carrier_p=0.3,
                        unphased_p=0.1, missing_p=0.03, haploid_p=0.0, chrom="c1", p_same=0.0, max_indel=4):
    """The "mix" recipe of SURVEY.md §4.5: SNPs, 1-4 bp insertions/deletions, two-ALT rows, MNPs, with a
    share of sites 1-3 bp from their predecessor.  Returns (fasta, vcf, names)."""
    rng = np.random.default_rng(seed)
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=ref_len))
    if sample_names is None:
        sample_names = [f"S{i + 1:03d}" for i in range(n_samples)]
    n_samples = len(sample_names)
    pos_list = []
    p = int(rng.integers(2, 20))
    while len(pos_list) < n_rows and p < ref_len - 12 - max_indel:
        pos_list.append(p)
        if p_same and rng.random() < p_same:
            continue  # another row at the very same position (repeated / split multi-allelic sites)
        if rng.random() < p_near:
            p += int(rng.integers(1, 4))
        else:
            p += int(rng.integers(4, max(5, 2 * (ref_len // max(n_rows, 1)))))
    fasta = os.path.join(dirpath, f"r{seed}.fa")
    vcf = os.path.join(dirpath, f"r{seed}.vcf")
    with open(fasta, "w") as f:
        f.write(f">{chrom} random\n")
        for i in range(0, ref_len, 60):
            f.write(ref[i:i + 60] + "\n")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(sample_names) + "\n")
        for p in pos_list:
            t = rng.random()
            r0 = ref[p - 1]
            if t < p_ins:
                k = int(rng.integers(1, max_indel + 1))
                refa, alts = r0, [r0 + "".join(BASES[i] for i in rng.integers(0, 4, size=k))]
            elif t < p_ins + p_del:
                k = int(rng.integers(1, max_indel + 1))
                refa, alts = ref[p - 1:p + k], [r0]
            elif t < p_ins + p_del + p_mnp:
                refa = ref[p - 1:p + 1]
                alts = ["".join(BASES[(BASES.index(c) + 1 + int(rng.integers(0, 3))) % 4] for c in refa)]
            else:
                refa = r0
                others = [b for b in BASES if b != r0]
                rng.shuffle(others)
                alts = [others[0]]
                if rng.random() < p_multi:
                    alts.append(others[1])
            gts = []
            any_car = False
            for s in range(n_samples):
                if rng.random() < missing_p:
                    gts.append("./.")
                    continue
                if haploid_p and rng.random() < haploid_p:
                    a = 1 if rng.random() < carrier_p else 0
                    gts.append(str(a))
                    any_car |= a > 0
                    continue
                a1 = int(rng.integers(1, len(alts) + 1)) if rng.random() < carrier_p else 0
                a2 = int(rng.integers(1, len(alts) + 1)) if rng.random() < carrier_p else 0
                sep = "/" if rng.random() < unphased_p else "|"
                gts.append(f"{a1}{sep}{a2}")
                any_car |= (a1 > 0 or a2 > 0)
            if not any_car:
                gts[int(rng.integers(0, n_samples))] = "1|0"
            f.write(f"{chrom}\t{p}\t.\t{refa}\t{','.join(alts)}\t99\t.\t.\tGT\t" + "\t".join(gts) + "\n")
    return fasta, vcf, sample_names


SAT_REF_LEN = 20_000


def write_saturated_cohort(dirpath, n_samples, seed, rows=150, two_alt=True, extremes=False, sparse_head=0):
    """FASTA + VCF (sat.fa, sat.vcf) of `rows` rows 120 - 129 bases apart (SNPs, 6 % insertions, 6 % deletions, 3 % two-ALT rows, a
    tenth of the carriers' calls moved on to 1|1, 1/0 or 1/1): row k is carried by all but k / 8 % 6 samples when k % 8 == 0 (rows 0,
    48, 96, 144: by every sample), else by a share of the samples drawn from [0.75, 0.99]; rows 4, 20, 36, ... keep only their
    carriers among samples 1..2015 (1,500 - 2,000 of them: dense at every threshold, and no carrier in the upper half of the row).
    VariantStore.synthetic caps an allele's frequency at 0.5, so rows like these exist only as VCF text.

    The options draw no random number, so the defaults and the rows they leave alone are the same bytes whatever they are:
      two_alt=False   the two-ALT records are written as SNPs of their first ALT
      extremes=True   the calls of rows 1..6 (single-ALT then) are overwritten: everybody 1/1, 1|1, 0|1, 1/0; everybody a carrier
                      but sample 1; everybody but the last sample.
      sparse_head=H   the calls of records 0..H-1 are thinned to max(1, n_samples // 50) carriers each, chosen by a generator of the
                      option's own (seeded from `seed`): a kept sample keeps its call, everybody else becomes 0|0, and if every kept
                      call is 0|0 one of them becomes 0|1.  Records H.. are untouched.  With H >= 100 the constructor, which looks
                      at the carrier density of the first 99 records, opens the cohort with EXPLICIT sample ids -- and then meets
                      carrier lists as long as the cohort.  extremes=True concerns rows 1..6, so it makes no sense together with
                      sparse_head > 6 (asserted)."""
    assert not (extremes and sparse_head > 6), "extremes rewrites rows 1..6, which sparse_head > 6 would thin again"
    rng = np.random.default_rng(seed)
    thin = np.random.default_rng([int(seed), 0x5EAD]) if sparse_head else None   # (never the writer's generator: the defaults' bytes stay)
    ref = "".join(BASES[i] for i in rng.integers(0, 4, size=SAT_REF_LEN))
    names = [f"S{i + 1:05d}" for i in range(n_samples)]
    one_alt = np.array(["0|0", "1|0", "0|1", "1|1", "1/0", "1/1"])
    two_alt_calls = np.array(["0|0", "1|0", "0|2", "2|1", "1|1", "2/2"])
    fasta, vcf = os.path.join(dirpath, "sat.fa"), os.path.join(dirpath, "sat.vcf")
    with open(fasta, "w") as f:
        f.write(">c1 saturated\n")
        for i in range(0, SAT_REF_LEN, 60):
            f.write(ref[i:i + 60] + "\n")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        p = 100
        for k in range(rows):
            p += int(rng.integers(120, 130))
            r0, t, calls = ref[p - 1], rng.random(), one_alt
            if t < 0.06:
                refa, alt = r0, r0 + "".join(BASES[i] for i in rng.integers(0, 4, size=int(rng.integers(1, 5))))
            elif t < 0.12:
                refa, alt = ref[p - 1:p + int(rng.integers(1, 5))], r0
            else:
                others = [b for b in BASES if b != r0]
                refa, alt = r0, others[int(rng.integers(0, 3))]
                if t < 0.15 and two_alt and not (extremes and 1 <= k <= 6):
                    alt, calls = alt + "," + [b for b in others if b != alt][0], two_alt_calls
            if k % 8 == 0:
                carrier = np.ones(n_samples, bool)
                carrier[rng.choice(n_samples, size=(k // 8) % 6, replace=False)] = False
            else:
                carrier = rng.random(n_samples) < rng.uniform(0.75, 0.99)
                if k % 16 == 4:
                    carrier[2015:] = False                            # ids 1..2015 only: nothing for the second half of a row
            call = np.where(carrier, rng.integers(1, 4, size=n_samples), 0)
            call[carrier & (rng.random(n_samples) < 0.1)] += 2        # calls 1..3 -> 3..5: still carriers
            if extremes and 1 <= k <= 4:
                call[:] = (5, 3, 2, 4)[k - 1]                         # 1/1, 1|1, 0|1, 1/0
            elif extremes and k in (5, 6):
                call = np.where(call == 0, 1 + np.arange(n_samples) % 5, call)
                call[0 if k == 5 else n_samples - 1] = 0
            if k < sparse_head:
                kept = thin.choice(n_samples, size=max(1, n_samples // 50), replace=False)
                thinned = np.zeros_like(call)
                thinned[kept] = call[kept]
                if not thinned.any():
                    thinned[kept[0]] = 2                               # 0|1
                call = thinned
            f.write(f"c1\t{p}\t.\t{refa}\t{alt}\t99\t.\t.\tGT\t" + "\t".join(calls[call]) + "\n")
    return fasta, vcf


def random_regions(rng, ref_len, n, max_len=600):
    """Random regions plus the edge shapes the reference's driver can be handed."""
    out = []
    for _ in range(n):
        x = int(rng.integers(1, ref_len + 1))
        out.append((x, x + int(rng.integers(0, max_len))))
    out += [(1, ref_len + 1), (1, ref_len), (1, ref_len + 100), (ref_len, ref_len + 5), (ref_len + 1, ref_len + 9),
            (ref_len + 50, ref_len + 60), (5, 5), (9, 3), (1, 2), (2, 3)]
    return out


def oracle_texts(orc, regions, sample=None):
    """[(n, early_out, text)] from the CPU oracle; n == -1 marks a non-terminating reference walk."""
    out = []
    for x, y in regions:
        if sample is None:
            out.append(orc.get_var_in_ref(x, y))
        else:
            out.append(orc.get_sample_var_in_ref(x, y, sample))
    return out


def read_plain(path):
    """Parse the plain dump (HostGraph::write_plain) into a dict of numpy arrays / lists."""
    import struct
    data = open(path, "rb").read()
    assert data[:8] == b"VSPLAIN1"
    pos = [8]

    def u64():
        v = struct.unpack_from("<Q", data, pos[0])[0]
        pos[0] += 8
        return v

    def s():
        n = u64()
        v = data[pos[0]:pos[0] + n].decode("latin-1")
        pos[0] += n
        return v

    def vec(dt):
        n = u64()
        a = np.frombuffer(data, dtype=dt, count=n, offset=pos[0]).copy()
        pos[0] += n * np.dtype(dt).itemsize
        return a

    g = {"chr": s(), "ref_length": u64(), "num_samples": u64(), "use_bit_vector": u64(), "num_classes": u64()}
    for k, dt in [("off", "<u4"), ("len", "<u4"), ("class_id", "<u4"), ("ref_index", "<u4"), ("car_begin", "<u8"),
                  ("car_flags", "u1"), ("car_index", "<u4"), ("car_sid", "<u4"), ("seq", "u1"), ("class_bits", "<u8")]:
        g[k] = vec(dt)
    g["sample_names"] = [s() for _ in range(u64())]
    g["topo_inplace"] = vec("u1")
    g["topo_val"] = vec("<u4")
    g["aux_lists"] = [vec("<u4") for _ in range(u64())]
    g["idx_pos"] = vec("<u4")
    g["node_list"] = vec("<u4")
    return g


# ---- windows of a synthetic cohort (tests/native/synth_windows.cpp): how the oracle gets to see the full-size indexes ----
_SYNTH_WINDOWS_EXE = None


def synth_windows(kw, wins, outdir):
    """Write FASTA + VCF of the windows [(lo, hi), ...] (1-based, inclusive) of the synthetic cohort `kw` (the keyword
    arguments of VariantStore.synthetic) into outdir/w<k>.fa / .vcf; returns the records written per window."""
    import subprocess
    import tempfile
    global _SYNTH_WINDOWS_EXE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if _SYNTH_WINDOWS_EXE is None:
        exe = os.path.join(tempfile.mkdtemp(prefix="vs_native_"), "synth_windows")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(root, "tests", "native", "synth_windows.cpp")])
        _SYNTH_WINDOWS_EXE = exe
    args = [str(kw[k]) for k in ("ref_length", "num_variants", "num_samples", "seed", "first_pos", "frac_ins", "frac_del", "frac_multi",
                                 "max_indel", "af_exponent")] + [str(kw.get("max_af", 0.5)), str(outdir)]
    out = subprocess.run([_SYNTH_WINDOWS_EXE] + args, input="".join(f"{a} {b}\n" for a, b in wins), text=True, capture_output=True, check=True)
    return [int(line.split()[3]) for line in out.stdout.strip().split("\n")]


def parse_rows(text, shift=0):
    """Rows of a region's print_var text as (pos + shift, ref, alt, samples)."""
    rows = []
    for line in text.split("\n")[1:]:
        if line:
            p, ref, alt, s = line.split("\t")
            rows.append((int(p) + shift, ref, alt, s))
    return rows


def window_oracle(outdir, k):
    """The small index of window k built through the product's VCF path on the host, and the oracle over it."""
    from oracle.oracle import Oracle
    from variantstore_amd import VariantStore
    w = VariantStore.from_vcf(os.path.join(outdir, f"w{k}.fa"), os.path.join(outdir, f"w{k}.vcf"), device=-1)
    plain = os.path.join(outdir, f"w{k}.bin")
    w.export_plain(plain)
    w.close()
    orc = Oracle(plain)
    return orc


# ---- two ranks on one GPU: the stand-in for RCCL (tests/native/fake_rccl.cpp), loaded by the engine through VS_RCCL_LIB ----
_FAKE_RCCL = None


def build_fake_rccl():
    """Compile tests/native/fake_rccl.cpp (hipcc: it copies device buffers through the HIP runtime) and return the library's path."""
    import subprocess
    import tempfile
    global _FAKE_RCCL
    if _FAKE_RCCL is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        lib = os.path.join(tempfile.mkdtemp(prefix="vs_native_"), "libfake_rccl.so")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-fPIC", "-shared", "-o", lib,
                               os.path.join(root, "tests", "native", "fake_rccl.cpp")])
        _FAKE_RCCL = lib
    return _FAKE_RCCL


def vcf_truth_cases(outdir, k, lo, edge=60):
    """Expected type-6 rows of window k's ISOLATED records, derived from the window's VCF TEXT alone (tests/vcf_truth.py: no
    from_vcf, no oracle), in the coordinates of the whole cohort: [(abs_pos, 'pos\\tref\\talt\\tsamples\\n'), ...].  Records within
    `edge` bases of the window's ends are left out (a neighbour outside the window could touch them)."""
    import vcf_truth as vt
    names, recs = vt.read_vcf(os.path.join(outdir, f"w{k}.vcf"))
    assert names == sorted(names)
    length = max(r[0] + len(r[1]) for r in recs) if recs else 0
    out = []
    for i, text in vt.expected_type6_rows(names, recs):
        pos, ref, _alts, _g = recs[i]
        if pos <= edge or pos + len(ref) >= length - edge:
            continue
        p, rest = text.split("\t", 1)
        out.append((int(p) + lo - 1, f"{int(p) + lo - 1}\t{rest}", recs[i]))
    return names, out

"""Trio queries on wide cohorts (vs_query_trio_scan): the forms of k_trio_scan<R> that tests/test_gpu_trio_scan.py never launches,
and the packed fields of the kernel at the maxima its comments state.

  1. every R, first and last pitch   a synthetic cohort of 65,600 samples; 3,073 to 65,536 member columns: k_trio_scan<16>, <8>, <4>,
                                     <2> and <1> at the first and the last pitch of their ranges -- the halving butterfly, the
                                     lane-to-row map and the zero-padded rows of a partial last row block in every form, tiles above
                                     48 KiB up to the full 64 KiB, the 16-byte store of a launch with ONE row block (a table of one
                                     row), trio_chunk 0, 64 and 16384; the refusal of 65,537 members
  2. the packed fields at their maxima a pedigree of 70 samples written as VCF text: 16,384, 16,385 and 32,833 DISTINCT trios that all
                                     add 2 to the same field of the same row -- a lane's 8-bit field at 128, a wave's 16-bit field at
                                     8,192, the workgroup's at 32,768 --, expected from the construction alone

Everything is compared bit for bit against trio_ref.trio_scan over the engine's own genotype_matrix() of the same regions and
members (test_gpu_trio_scan._check_full); trio_ref computes the closed forms and the gamete enumeration and asserts they agree."""
import os
import time

import numpy as np
import pytest

from test_gpu_trio_scan import VS_ERR_ARG, VS_ERR_UNSUPPORTED, _check_full, _row_keys, make_trios
from trio_ref import FIELDS
from variantstore_amd import VariantStore
from variantstore_amd.api import VariantStoreError

pytestmark = pytest.mark.gpu
CHUNK_MAX = 16384                # kTrioChunkMax: 64 slabs of 64 trios for each of a workgroup's four waves
ROWS_MAX, TILE_BYTES = 16, 64 << 10


def _expected_rows_per_block(pitch):
    """The engine's rule: the largest power of two up to min(16, 64 KiB / pitch), at least 1."""
    r = ROWS_MAX
    while r > 1 and r * pitch > TILE_BYTES:
        r >>= 1
    return r


def _same_under_every_chunk(vs, regions, trios, chunks, what, conditions):
    """The batch under every trio_chunk of `chunks`: the first through _check_full (every record against trio_ref over the matrix),
    the others against the same reference records and, byte for byte, against the first.  Returns (matrix arrays, expected, first
    result)."""
    first = None
    try:
        for chunk in chunks:
            vs.set_option("trio_chunk", chunk)
            if first is None:
                m, want, first = _check_full(vs, regions, trios, (what, chunk), conditions=conditions)
                continue
            res = vs.trio_scan(regions, trios)
            got = res.trio_scan()
            res.close()
            for f in FIELDS:   # against the reference ...
                bad = np.nonzero(got["trio_stats"][f] != want["trio_stats"][f])[0]
                assert bad.shape[0] == 0, (what, chunk, "trio", f, bad[:8].tolist(), got["trio_stats"][f][bad[:8]].tolist(), want["trio_stats"][f][bad[:8]].tolist())
            assert _row_keys(got["rows"], got["row_stats"]) == _row_keys(m["rows"], want["row_stats"]), (what, chunk)
            assert got["n_used"] == want["n_used"], (what, chunk)
            # ... and the bytes of the first (only integer adds: the chunk changes nothing)
            assert got["rows"].tobytes() == first["rows"].tobytes(), (what, chunk)
            assert got["row_stats"].tobytes() == first["row_stats"].tobytes(), (what, chunk, "row_stats")
            assert got["trio_stats"].tobytes() == first["trio_stats"].tobytes(), (what, chunk, "trio_stats")
            assert got["n_used"] == first["n_used"] and got["counts"].tobytes() == first["counts"].tobytes(), (what, chunk)
    finally:
        vs.set_option("trio_chunk", 0)
    return m, want, first


# --------------------------------------------------------------------- 1. every R, at the first and the last pitch of its range
WIDE_SAMPLES = 65_600
WIDE_KW = dict(ref_length=60_000, num_variants=300, num_samples=WIDE_SAMPLES, seed=91, first_pos=100, frac_ins=0.06, frac_del=0.06,
               frac_multi=0.03, max_indel=4, af_exponent=1.0)
# ids every draw of members includes: the first and the last of the cohort, both sides of the first mask-word boundary (63 | 64) and
# of the boundary between mask words 63 and 64 (4,095 | 4,096)
EDGE_IDS = (1, 63, 64, 4095, 4096, WIDE_SAMPLES)
# members -> (pitch, R, tile bytes)
WIDE_CASES = {3_073: (3_088, 16, 49_408),    # the first tile above 48 KiB
              4_096: (4_096, 16, 65_536),    # the full tile, the last R = 16
              4_097: (4_112, 8, 32_896),     # the first R = 8
              8_192: (8_192, 8, 65_536),
              8_193: (8_208, 4, 32_832),
              16_385: (16_400, 2, 32_800),
              32_768: (32_768, 2, 65_536),
              32_769: (32_784, 1, 32_784),
              65_536: (65_536, 1, 65_536)}   # the limit


class _WideSynth:
    """The synthetic cohort, opened once; a handful of unsorted regions whose table has an odd number of rows in 33 .. 80, and one
    region whose table is ONE row."""

    def __init__(self):
        t0 = time.perf_counter()
        self.vs = VariantStore.synthetic(device=0, **WIDE_KW)
        self.open_seconds = time.perf_counter() - t0
        print(f"VariantStore.synthetic with {WIDE_SAMPLES} samples and {WIDE_KW['num_variants']} variants: {self.open_seconds:.2f} s")
        vs = self.vs
        assert vs.info().num_samples - 1 == WIDE_SAMPLES
        L = vs.info().ref_length
        probe = vs.allele_counts([(1, L)])
        ac = probe.allele_counts()
        probe.close()
        pos = np.unique(ac["rows"]["pos"].astype(np.int64))
        assert pos.shape[0] > 200
        # candidates: disjoint stretches of 4 .. 9 consecutive record positions, in a shuffled order.  With seed 91 the search below
        # ends at the eight regions (5061, 5581), (38573, 39189), (31247, 32245), (26597, 27622), (16971, 18034), (33701, 34851),
        # (50408, 51343), (2579, 4287) -- 2 + 3 + 4 + 4 + 4 + 6 + 3 + 7 = 33 rows -- and the one-row region (52032, 52034).
        rng = np.random.default_rng(17)
        cands = [(int(pos[k]), int(pos[k + int(rng.integers(3, 9))])) for k in range(0, pos.shape[0] - 12, 12)]
        cands = [cands[i] for i in rng.permutation(len(cands))]

        def table_rows(regions):
            res = vs.allele_counts(regions)
            n = int(res.allele_counts()["rows"].shape[0])
            res.close()
            return n
        chosen = []
        while table_rows(chosen + [cands[len(chosen)]]) < 30:
            chosen.append(cands[len(chosen)])
        last = [c for c in cands[len(chosen):] if table_rows(chosen + [c]) in range(33, 46, 2)]   # (the reference's cost grows with the rows)
        assert last, "no candidate completes an odd table of 33 .. 45 rows"
        self.regions = chosen + [last[0]]
        self.table_rows = table_rows(self.regions)
        assert len(self.regions) >= 4 and self.regions != sorted(self.regions), self.regions
        # one region of ONE row, a common one (every state of a trio occurs in it): among the positions with a single record the one
        # whose alternate-allele count is nearest to the number of samples, an allele frequency of one half
        single = [int(p) for p in pos if int((ac["rows"]["pos"] == p).sum()) == 1]
        order = sorted(single, key=lambda p: abs(int(ac["counts"]["alt_alleles"][ac["rows"]["pos"] == p][0]) - WIDE_SAMPLES))
        one = [p for p in order[:20] if table_rows([(p - 1, p + 1)]) == 1]   # (a region's ends are exclusive)
        assert one, "no region of one row"
        self.one_row = [(one[0] - 1, one[0] + 1)]
        print(f"regions {self.regions}: a table of {self.table_rows} rows; the one-row region {self.one_row}")


@pytest.fixture(scope="module")
def wide():
    w = _WideSynth()
    yield w
    w.vs.close()


def _members(n, seed):
    """n sorted ids of the cohort drawn with a fixed seed, the edge ids among them."""
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(1, WIDE_SAMPLES + 1), EDGE_IDS)
    out = np.sort(np.concatenate([np.asarray(EDGE_IDS), rng.choice(rest, size=n - len(EDGE_IDS), replace=False)]))
    assert out.shape[0] == n == np.unique(out).shape[0] and all(e in out for e in EDGE_IDS)
    return out


@pytest.mark.parametrize("n_members", list(WIDE_CASES), ids=[f"{n}-pitch{p}-R{r}-tile{t}" for n, (p, r, t) in WIDE_CASES.items()])
def test_every_rows_per_block_at_both_ends_of_its_range(n_members, wide):
    """k_trio_scan<R> for R = 16, 8, 4, 2 and 1 at the first and the last pitch that selects it: ceil(members / 3) + 37 trios (every
    member column is read, the count is no multiple of 64) over a table with an odd number of rows (a partial last row block for
    R = 16, 8, 4 and 2: zero-padded rows in the unrolled loop, `tid < n_rows` in the epilogue) and over a table of ONE row (one row
    block: the trios leave by the 16-byte store, the only way to it at R = 1), each under trio_chunk 0 (by the shape), 64 (hundreds of
    chunks: the atomic row path) and 16384 (one or two chunks of 64 slabs a wave)."""
    pitch, rows_per_block, tile = WIDE_CASES[n_members]
    vs = wide.vs
    members = _members(n_members, 5000 + n_members)
    n_trios = (n_members + 2) // 3 + 37
    assert n_trios % 64 != 0
    trios = make_trios(members, n_trios, np.random.default_rng(n_members))
    assert np.unique(trios).shape[0] == n_members
    t0 = time.perf_counter()
    m, want, got = _same_under_every_chunk(vs, wide.regions, trios, (0, 64, CHUNK_MAX), n_members, conditions=True)
    a = m["cells"].shape[0]
    assert 33 <= a <= 80 and a % 2 == 1 and a == wide.table_rows, a
    assert m["cells"].shape[1] == n_members and m["columns"].tolist() == members.tolist()
    # the form this case is about, from the pitch the engine reports -- a changed rule must not turn it into R = 16 again
    assert m["row_pitch"] == pitch == (n_members + 15) // 16 * 16
    assert _expected_rows_per_block(m["row_pitch"]) == rows_per_block and rows_per_block * m["row_pitch"] == tile <= TILE_BYTES
    if rows_per_block > 1:
        assert a % rows_per_block != 0, "the last row block is not partial"
    assert want["row_stats"]["errors"].any() and want["row_stats"]["transmitted"].any() and want["trio_stats"]["untransmitted"].any()
    m1, want1, _got1 = _same_under_every_chunk(vs, wide.one_row, trios, (0, 64, CHUNK_MAX), (n_members, "one row"), conditions=False)
    assert m1["cells"].shape == (1, n_members) and m1["row_pitch"] == pitch
    assert all(int(want1["row_stats"][f][0]) > 0 for f in FIELDS), want1["row_stats"]
    print(f"{n_members} members, pitch {pitch}, R = {rows_per_block}, tile {tile} bytes, {n_trios} trios, {a} rows and 1 row: {time.perf_counter() - t0:.2f} s")


def test_one_member_above_the_limit_is_refused(wide):
    """65,537 members: VS_ERR_UNSUPPORTED before anything is allocated, both numbers in the message; the handle answers the next
    batch as before."""
    vs = wide.vs
    rng = np.random.default_rng(3)
    n = TILE_BYTES + 1
    trios = make_trios(np.arange(1, n + 1), (n + 2) // 3 + 37, rng)
    assert np.unique(trios).shape[0] == 65_537 and int(trios.max()) == 65_537
    before = vs.info().pool_mallocs
    with pytest.raises(VariantStoreError) as e:
        vs.trio_scan(wide.regions, trios)
    assert e.value.code == VS_ERR_UNSUPPORTED
    assert "65537" in str(e.value) and "65536" in str(e.value), str(e.value)
    assert vs.info().pool_mallocs == before, "a refused batch allocated"
    members = _members(300, 11)
    m, _want, _got = _check_full(vs, wide.regions, make_trios(members, 137, rng), "after the refusal")
    assert m["cells"].shape == (wide.table_rows, 300)


# ----------------------------------------------------------------------------------- 2. the packed fields at their stated maxima
N_KIDS, N_PARENTS, PED_ROWS, PED_REF_LEN = 40, 30, 16, 2_000
PLANTED = {"T": 6, "U": 7, "E": 8, "F": 9}   # the table rows of the planted records: neighbours, so that one region holds just the four
# trios -> the planted rows' expected sums, from the construction: 2 n transmitted, 2 n untransmitted, (n, n) errors and de novo
# calls, (n, 0) errors
PLANTED_SUMS = {16_384: {"T": 32_768, "U": 32_768, "E": (16_384, 16_384), "F": (16_384, 0)},
                16_385: {"T": 32_770, "U": 32_770, "E": (16_385, 16_385), "F": (16_385, 0)},
                32_833: {"T": 65_666, "U": 65_666, "E": (32_833, 32_833), "F": (32_833, 0)}}
PLANTED_TRIO_RECORD = (2, 1, 2, 2)   # every trio over the four planted rows: E and F are errors, E a de novo call, T = 2 and U = 2


def write_field_pedigree(dirpath, seed=23):
    """FASTA + VCF of 40 "kids" and 30 "parents", 16 single-ALT rows 55 bases apart; four of them planted, the others random:
      T row  every kid 1/1, every parent 0/1: whatever (kid, parent, parent) a trio names, it adds T = 2
      U row  every kid 0/0, every parent 0/1: U = 2
      E row  every kid 1/1, every parent 0/0: an error and a de novo call
      F row  every kid 0/0, every parent 1/1: an error, no de novo call
    Returns (fasta, vcf, kid names, parent names, positions)."""
    rng = np.random.default_rng(seed)
    bases = "ACGT"
    ref = "".join(bases[i] for i in rng.integers(0, 4, size=PED_REF_LEN))
    kids, parents = [f"K{k:02d}" for k in range(N_KIDS)], [f"P{p:02d}" for p in range(N_PARENTS)]   # (ascending in the columns' order)
    planted = {PLANTED["T"]: ("1/1", "0/1"), PLANTED["U"]: ("0/0", "0/1"), PLANTED["E"]: ("1/1", "0/0"), PLANTED["F"]: ("0/0", "1/1")}
    positions = [50 + 55 * r for r in range(PED_ROWS)]
    fasta, vcf = os.path.join(dirpath, "fields.fa"), os.path.join(dirpath, "fields.vcf")
    with open(fasta, "w") as f:
        f.write(">c1 fields\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, PED_REF_LEN, 60)))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(kids + parents) + "\n")
        for r, p in enumerate(positions):
            if r in planted:
                calls = [planted[r][0]] * N_KIDS + [planted[r][1]] * N_PARENTS
            else:   # every dosage about as often, phased and not
                calls = [("0|0", "0|1", "1|0", "1|1", "0/1", "1/1")[i] for i in rng.integers(0, 6, size=N_KIDS + N_PARENTS)]
            r0 = ref[p - 1]
            f.write(f"c1\t{p}\t.\t{r0}\t{bases[(bases.index(r0) + 1) % 4]}\t99\t.\t.\tGT\t" + "\t".join(calls) + "\n")
    return fasta, vcf, kids, parents, positions


@pytest.fixture(scope="module")
def field_pedigree(tmp_path_factory):
    fasta, vcf, kids, parents, positions = write_field_pedigree(str(tmp_path_factory.mktemp("trio_fields")))
    vs = VariantStore.from_vcf(fasta, vcf, device=0)
    kid_ids, parent_ids = [vs.sample_id(x) for x in kids], [vs.sample_id(x) for x in parents]
    assert sorted(kid_ids + parent_ids) == list(range(1, N_KIDS + N_PARENTS + 1))
    # every (kid, parent i, parent j), i != j: 40 x 30 x 29 distinct triples of distinct ids, in a shuffled order
    every = np.asarray([(k, f, m) for k in kid_ids for f in parent_ids for m in parent_ids if f != m], np.uint32)
    assert every.shape == (34_800, 3) and np.unique(every, axis=0).shape[0] == 34_800
    every = every[np.random.default_rng(29).permutation(every.shape[0])]
    yield vs, every, positions
    vs.close()


@pytest.mark.parametrize("n_trios", list(PLANTED_SUMS))
def test_packed_fields_at_their_maxima(n_trios, field_pedigree):
    """Under trio_chunk = 16384, 16,384 trios are ONE chunk of 64 slabs a wave: on the T row every lane adds 2 to the same 8-bit field
    64 times (128 < 256), the wave's 16-bit field holds 64 x 128 = 8,192 behind the butterfly and the four waves' sum is 32,768
    (< 65,536), written with a plain store; the U, E and F rows do the same to the other three fields.  16,385 trios add a chunk of one
    lane (the atomic row path), 32,833 = 2 x 16,384 + 65 two full chunks and a remainder.  A lost carry in the widening or a chunk
    above 16,384 trios shows in the planted rows, whose sums are written out above."""
    vs, every, positions = field_pedigree
    trios = every[:n_trios]
    sums = PLANTED_SUMS[n_trios]
    whole = [(1, PED_REF_LEN)]
    m, want, got = _same_under_every_chunk(vs, whole, trios, (CHUNK_MAX, 64, 0), ("fields", n_trios), conditions=True)
    assert got["rows"]["pos"].tolist() == positions and got["n_used"] == PED_ROWS and m["row_pitch"] == 80
    rec = got["row_stats"]
    assert tuple(int(rec[f][PLANTED["T"]]) for f in FIELDS) == (0, 0, sums["T"], 0) and sums["T"] == 2 * n_trios
    assert tuple(int(rec[f][PLANTED["U"]]) for f in FIELDS) == (0, 0, 0, sums["U"]) and sums["U"] == 2 * n_trios
    assert tuple(int(rec[f][PLANTED["E"]]) for f in FIELDS) == sums["E"] + (0, 0) and sums["E"] == (n_trios, n_trios)
    assert tuple(int(rec[f][PLANTED["F"]]) for f in FIELDS) == sums["F"] + (0, 0) and sums["F"] == (n_trios, 0)
    others = [r for r in range(PED_ROWS) if r not in PLANTED.values()]
    assert np.unique(rec[others]).shape[0] == len(others), "the random rows are not uniform"
    # the four planted rows alone: every trio's record is the same constant
    four = [(positions[PLANTED["T"]] - 20, positions[PLANTED["F"]] + 20)]
    m4, _want4, got4 = _same_under_every_chunk(vs, four, trios, (CHUNK_MAX, 64, 0), ("planted rows", n_trios), conditions=False)
    assert got4["rows"]["pos"].tolist() == positions[PLANTED["T"]:PLANTED["F"] + 1] and m4["cells"].shape == (4, N_KIDS + N_PARENTS)
    assert np.array_equal(got4["row_stats"], rec[PLANTED["T"]:PLANTED["F"] + 1])
    constant = np.zeros(n_trios, got4["trio_stats"].dtype)
    for f, v in zip(FIELDS, PLANTED_TRIO_RECORD):
        constant[f] = v
    assert got4["trio_stats"].tobytes() == constant.tobytes()


def test_a_chunk_above_the_stated_maximum_is_refused(field_pedigree):
    """The bounds above hold for 64 slabs a wave: trio_chunk takes nothing above 16,384 trios."""
    vs, _every, _positions = field_pedigree
    try:
        for chunk in (CHUNK_MAX + 64, 2 * CHUNK_MAX):
            with pytest.raises(VariantStoreError) as e:
                vs.set_option("trio_chunk", chunk)
            assert e.value.code == VS_ERR_ARG and "16384" in str(e.value), str(e.value)
        vs.set_option("trio_chunk", CHUNK_MAX)
    finally:
        vs.set_option("trio_chunk", 0)

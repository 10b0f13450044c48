"""Trio queries without a GPU: the reference's two computations against each other -- on all 27 states, one cell each, on a
hand-worked example and on random matrices --, the random cohorts the GPU test opens (that they show every state, from the VCF text
alone), the argument checks of vs_query_trio_scan (made on the host, before the handle's device is asked for) and their order, the
host-only refusal, the Python wrapper's codes, and the CLI's usage errors and trio-file parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import write_random_cohort
from trio_ref import (FIELDS, TRIO_DTYPE, dosage, error_rate, state_by_enumeration, state_closed_form, states, tdt_chi2, trio_scan,
                      trio_table_text, trio_text)
from variantstore_amd import VariantStore, _lib, trio_error_rate, trio_tdt_chi2
from variantstore_amd.api import QueryResult, VariantStoreError

VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE, VS_ERR_UNSUPPORTED = -3, -5, -6, -7
VS_TRIOS_MAX = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
CELL_OF_DOSAGE = np.asarray([0, 2, 7], np.uint8)   # 0, 1|0, 1|1 phased


# ------------------------------------------------------------------------------------------------------ the reference itself
def test_all_27_states_one_cell_each():
    """The semantics table, written out by hand, against both computations."""
    want = {  # (f, m): per child dosage 0, 1, 2 -> (error, denovo, T, U)
        (0, 0): [(0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0)],
        (0, 1): [(0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 0)],
        (0, 2): [(1, 0, 0, 0), (0, 0, 0, 0), (1, 0, 0, 0)],
        (1, 0): [(0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 0)],
        (1, 1): [(0, 0, 0, 2), (0, 0, 1, 1), (0, 0, 2, 0)],
        (1, 2): [(1, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)],
        (2, 0): [(1, 0, 0, 0), (0, 0, 0, 0), (1, 0, 0, 0)],
        (2, 1): [(1, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0)],
        (2, 2): [(1, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0)],
    }
    n_err = 0
    for f in range(3):
        for m in range(3):
            for c in range(3):
                rec = want[(f, m)][c]
                assert state_by_enumeration(f, m, c) == rec == state_closed_form(f, m, c), (f, m, c)
                cells = CELL_OF_DOSAGE[np.asarray([[c, f, m]])]
                got = trio_scan(cells, [(0, 1, 2)])
                for k, name in enumerate(FIELDS):
                    assert int(got["row_stats"][name][0]) == rec[k] == int(got["trio_stats"][name][0]), (f, m, c, name)
                assert got["n_used"] == 1 and int(states(cells, [(0, 1, 2)])[0, 0]) == 9 * f + 3 * m + c
                n_err += rec[0]
    assert n_err == 12   # of 27
    # every storage form of a dosage gives the same answer: 2 / 4 (one allele, either slot), 3 / 5 (the same, phase bit set), 6 / 7
    assert dosage(np.asarray([0, 1, 2, 3, 4, 5, 6, 7], np.uint8)).tolist() == [0, 0, 1, 1, 1, 1, 2, 2]


def test_reference_on_a_hand_worked_example():
    # columns: 0 child A, 1 father, 2 mother, 3 child B (of the same parents), 4 a parent of nobody but a child of (1, 2) too
    d = np.asarray([[1, 1, 0, 0, 2],     # A consistent (T 1, U 0 from the father); B consistent (T 0, U 1); col 4: error
                    [2, 1, 1, 1, 0],     # A T 2 U 0; B T 1 U 1; col 4 T 0 U 2
                    [1, 0, 0, 0, 0],     # A de novo; B and col 4 nothing
                    [0, 0, 0, 0, 0],     # dropped
                    [0, 2, 2, 2, 1]])    # A error (not de novo); B consistent, no het parent; col 4 error
    cells = CELL_OF_DOSAGE[d]
    dropped = np.asarray([0, 0, 0, 1, 0], bool)
    trios = [(0, 1, 2), (3, 1, 2), (4, 1, 2), (0, 1, 2)]   # the first trio twice: it counts twice
    w = trio_scan(cells, trios, dropped)
    assert w["n_used"] == 4 and w["row_stats"].dtype == TRIO_DTYPE and w["trio_stats"].dtype == TRIO_DTYPE
    assert w["row_stats"]["errors"].tolist() == [1, 0, 2, 0, 3] and w["row_stats"]["denovo"].tolist() == [0, 0, 2, 0, 0]
    assert w["row_stats"]["transmitted"].tolist() == [2, 5, 0, 0, 0] and w["row_stats"]["untransmitted"].tolist() == [1, 3, 0, 0, 0]
    assert w["trio_stats"]["errors"].tolist() == [2, 0, 2, 2] and w["trio_stats"]["denovo"].tolist() == [1, 0, 0, 1]
    assert w["trio_stats"]["transmitted"].tolist() == [3, 1, 0, 3] and w["trio_stats"]["untransmitted"].tolist() == [0, 2, 2, 0]
    chi = tdt_chi2(w["row_stats"])
    assert chi[:2].tolist() == [1.0 / 3.0, 4.0 / 8.0] and np.isnan(chi[2:]).all()
    assert error_rate(w["trio_stats"], w["n_used"]).tolist() == [0.5, 0.0, 0.5, 0.5] and np.isnan(error_rate(w["trio_stats"], 0)).all()
    # the package's derived quantities are the reference's, bit for bit
    assert trio_tdt_chi2(w["row_stats"]).tobytes() == chi.tobytes()
    assert trio_error_rate(w["trio_stats"], 4).tobytes() == error_rate(w["trio_stats"], 4).tobytes() and np.isnan(trio_error_rate(w["trio_stats"], 0)).all()
    with pytest.raises(AssertionError):
        trio_scan(cells, trios, np.asarray([1, 0, 0, 0, 0], bool))   # a dropped row with a set cell
    e = trio_scan(cells[:0], trios)
    assert e["n_used"] == 0 and e["row_stats"].shape == (0,) and e["trio_stats"].shape == (4,) and not e["trio_stats"].view(np.uint32).any()
    heads = [f"{10 * i}\tA\tC" for i in range(5)]
    ac = dosage(cells).sum(axis=1)
    assert trio_text(heads, ac, w["row_stats"], dropped) == ("Pos\tRef\tAlt\tAC\tErrors\tDeNovo\tT\tU\n0\tA\tC\t4\t1\t0\t2\t1\n10\tA\tC\t5\t0\t0\t5\t3\n"
                                                            "20\tA\tC\t1\t2\t2\t0\t0\n40\tA\tC\t7\t3\t0\t0\t0\n")
    assert trio_table_text([("a", "f", "m"), ("b", "f", "m")], w["trio_stats"][:2], 4) == ("Child\tFather\tMother\tN\tErrors\tDeNovo\tT\tU\n"
                                                                                         "a\tf\tm\t4\t2\t1\t3\t0\nb\tf\tm\t4\t0\t0\t1\t2\n")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_computations_agree_on_random_matrices(seed):
    """trio_scan asserts its closed forms against the enumeration; here on random cells of every storage pattern, with dropped rows
    and members in several roles, and the invariants that follow."""
    rng = np.random.default_rng(seed)
    n, t_n = (23, 64, 7)[seed - 1], (40, 257, 5)[seed - 1]
    cells = rng.choice(np.asarray([0, 2, 4, 6, 7, 3, 5], np.uint8), size=(300, n), p=[0.4, 0.15, 0.15, 0.12, 0.12, 0.03, 0.03])
    dropped = rng.random(300) < 0.05
    cells[dropped] = 0
    trios = np.asarray([rng.choice(n, size=3, replace=False) for _ in range(t_n)])
    w = trio_scan(cells, trios, dropped)
    assert w["n_used"] == 300 - int(dropped.sum()) and dropped.any()
    assert np.unique(states(cells, trios)).shape[0] == 27
    r, t = w["row_stats"], w["trio_stats"]
    for f in FIELDS:
        assert int(r[f].astype(np.int64).sum()) == int(t[f].astype(np.int64).sum()) > 0, f
    assert (r["denovo"] <= r["errors"]).all() and (t["denovo"] <= t["errors"]).all() and not r["errors"][dropped].any()
    d = dosage(cells)
    het_parents = ((d[:, trios[:, 1]] == 1).astype(np.int64) + (d[:, trios[:, 2]] == 1)).sum(axis=1)
    assert (r["transmitted"].astype(np.int64) + r["untransmitted"] <= het_parents).all()   # (equal but for the error cells)


@pytest.mark.parametrize("seed,n_samples,n_rows,least", [(4101, 9, 120, 4), (4103, 66, 120, 30), (4101, 9, 400, 12), (4103, 66, 400, 100)])
def test_the_gpu_tests_cohorts_show_every_state(seed, n_samples, n_rows, least, tmp_path):
    """From the VCF text alone: with trios (1, 2, 3), (4, 5, 6), ... random cohorts with carrier_p = 0.5 show each of the 27 states at
    least `least` times -- at the writer's default of 120 records and at the 400 the GPU test's cohorts have; a single trio over
    three samples (seed 4102, 120 records) misses two of them, which is why the GPU test asserts the 27 states on cases of three
    trios or more (and takes its three columns from a cohort of nine: in a cohort of three no row has three non-carriers)."""
    def state_counts(seed, n_samples, n_rows=120):
        _fa, vcf, _names = write_random_cohort(os.path.join(tmp_path), seed, ref_len=6000, n_rows=n_rows, n_samples=n_samples, carrier_p=0.5)
        rows = []
        for line in open(vcf):
            if line.startswith("#"):
                continue
            f = line.rstrip("\n").split("\t")
            for k in range(1, len(f[4].split(",")) + 1):
                rows.append([g.replace("|", "/").split("/").count(str(k)) for g in f[9:]])
        d = np.asarray(rows)
        trios = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(n_samples // 3)]
        return np.bincount(np.concatenate([9 * d[:, f] + 3 * d[:, m] + d[:, c] for c, f, m in trios]), minlength=27)
    assert state_counts(seed, n_samples, n_rows).min() >= least
    assert int((state_counts(4102, 3) == 0).sum()) == 2


# ------------------------------------------------------------------------------------------------------ the C ABI on the host
@pytest.fixture(scope="module")
def host_store(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trio_host"))
    fasta, vcf, _names = write_random_cohort(d, 4101, ref_len=6000, n_samples=9, carrier_p=0.5)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    yield vs
    vs.close()


def _call(vs, trios, n_trios=None, n=1):
    lib = _lib.load()
    regions = (_lib.Region * 1)(_lib.Region(1, 100))
    h = C.c_void_p()
    flat = None if trios is None else [int(x) for t in trios for x in t]
    ptr = None if flat is None else (C.c_uint32 * max(len(flat), 1))(*flat)
    n_trios = (0 if trios is None else len(trios)) if n_trios is None else n_trios
    return lib.vs_query_trio_scan(vs._h, regions, n, ptr, n_trios, C.byref(h))


def _err():
    return _lib.load().vs_last_error().decode()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_trio_scan", "vs_result_get_trio_scan", "vs_result_trio_scan_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    assert "#define VS_TRIOS_MAX (1u << 20)" in header
    assert "typedef struct { uint32_t errors, denovo, transmitted, untransmitted; } vs_trio_counts;" in header
    assert QueryResult.TRIO_DTYPE == TRIO_DTYPE and TRIO_DTYPE.itemsize == 16


def test_host_only_handle_refuses_trios(host_store):
    assert host_store.info().num_samples == 10
    for trios in ([(1, 2, 3)], [(3, 2, 1), (1, 2, 3), (1, 2, 3)], [(9, 8, 7), (7, 1, 9)]):
        assert _call(host_store, trios) == VS_ERR_NO_DEVICE
        with pytest.raises(VariantStoreError) as e:
            host_store.trio_scan([(1, 100)], trios)
        assert e.value.code == VS_ERR_NO_DEVICE


def test_argument_errors_and_their_order(host_store):
    ns = host_store.info().num_samples
    # the batch
    assert _call(host_store, [(1, 2, 3)], n=0) == VS_ERR_ARG
    assert "region" in _err()
    # the trio table: NULL, none, too many
    assert _call(host_store, None) == VS_ERR_ARG
    assert "trios" in _err()
    assert _call(host_store, None, n_trios=4) == VS_ERR_ARG
    assert _call(host_store, [], n_trios=0) == VS_ERR_ARG          # a non-NULL pointer to no trios
    assert "0 trios" in _err()
    assert _call(host_store, [(1, 2, 3)], n_trios=VS_TRIOS_MAX + 1) == VS_ERR_ARG
    assert str(VS_TRIOS_MAX + 1) in _err()
    # two equal ids inside a triple: the message names the trio
    for bad in ((4, 4, 5), (4, 5, 4), (5, 4, 4), (6, 6, 6)):
        assert _call(host_store, [(1, 2, 3), (7, 8, 9), bad, (1, 2, 3)]) == VS_ERR_ARG, bad
        assert "trio 2 " in _err()
    # unknown ids
    for bad in ((0, 1, 2), (1, 0, 2), (1, 2, 0), (ns, 1, 2), (1, 2, 0xFFFFFFFF)):
        assert _call(host_store, [(1, 2, 3), bad]) == VS_ERR_UNKNOWN_SAMPLE, bad
        assert "trio 1" in _err()
    # the order: regions < NULL < the number < (per trio: equal ids < unknown ids) < the device
    assert _call(host_store, None, n=0) == VS_ERR_ARG
    assert "region" in _err()
    assert _call(host_store, None, n_trios=VS_TRIOS_MAX + 1) == VS_ERR_ARG
    assert "null" in _err()
    assert _call(host_store, [(0, 0, 1)], n_trios=VS_TRIOS_MAX + 1) == VS_ERR_ARG
    assert str(VS_TRIOS_MAX + 1) in _err()
    assert _call(host_store, [(0, 0, 1)]) == VS_ERR_ARG                                  # equal before unknown, inside one trio
    assert _call(host_store, [(0, 1, 2), (3, 3, 4)]) == VS_ERR_UNKNOWN_SAMPLE            # trio by trio: trio 0 is reported first
    assert _call(host_store, [(1, 2, 3), (3, 3, 4), (0, 1, 2)]) == VS_ERR_ARG
    assert _call(host_store, [(1, 2, 3)]) == VS_ERR_NO_DEVICE


def test_wrapper_raises_the_same_codes(host_store):
    names = [host_store.sample_name(i) for i in range(1, 10)]
    cases = (([], VS_ERR_ARG), ([(1, 1, 2)], VS_ERR_ARG), ([(0, 1, 2)], VS_ERR_UNKNOWN_SAMPLE), (np.asarray([[1, 2, 10]]), VS_ERR_UNKNOWN_SAMPLE),
             ([(names[0], names[1], names[0])], VS_ERR_ARG), ([(names[0], 2, names[2])], VS_ERR_NO_DEVICE),
             (np.asarray([[1, 2, 3], [4, 5, 6]], np.int64), VS_ERR_NO_DEVICE))
    for trios, code in cases:
        with pytest.raises(VariantStoreError) as e:
            host_store.trio_scan([(1, 100)], trios)
        assert e.value.code == code, trios
    with pytest.raises(VariantStoreError):
        host_store.trio_scan([(1, 100)], [(names[0], "no-such-sample", names[1])])
    for bad in ([(1, 2)], np.zeros((2, 4), np.uint32), [1, 2, 3]):
        with pytest.raises((ValueError, TypeError)):
            host_store.trio_scan([(1, 100)], bad)
    with pytest.raises(VariantStoreError) as e:
        host_store.trio_scan([], [(1, 2, 3)])
    assert e.value.code == VS_ERR_ARG
    assert host_store.trio_ids([(names[4], 2, names[8])]).tolist() == [[5, 2, 9]]
    for bad in (63, 65, 96, 16384 + 64, -1):
        with pytest.raises(VariantStoreError) as e:
            host_store.set_option("trio_chunk", bad)
        assert e.value.code == VS_ERR_ARG
    for ok in (64, 128, 16384, 0):
        host_store.set_option("trio_chunk", ok)


# ------------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_usage_errors_and_trio_files(tmp_path):
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    fasta, vcf, names = write_random_cohort(str(tmp_path), 4101, ref_len=6000, n_samples=9, carrier_p=0.5)
    subprocess.run([CLI, "construct", "-r", fasta, "-v", vcf, "-p", prefix], check=True, capture_output=True)
    tfile = os.path.join(tmp_path, "trios.txt")

    def run(text, *more):
        with open(tfile, "w") as f:
            f.write(text)
        return subprocess.run([CLI, "trios", "-p", prefix, "-r", "1:100", "-T", tfile, "--device", "-1", *more], capture_output=True, text=True)

    for argv in (["-p", prefix, "-r", "1:100"], ["-p", prefix, "-T", tfile], ["-r", "1:100", "-T", tfile], []):   # something is missing: the usage
        p = subprocess.run([CLI, "trios"] + argv, capture_output=True, text=True)
        assert p.returncode != 0 and "variantstore trios" in p.stdout and "--per-trio" in p.stdout and "PED" in p.stdout, argv
    p = subprocess.run([CLI, "trios", "-p", prefix, "-r", "1:100", "-T", tfile, "--king"], capture_output=True, text=True)   # another command's flag
    assert p.returncode != 0 and "unknown option" in p.stdout + p.stderr
    p = subprocess.run([CLI, "trios", "-p", prefix, "-r", "1:100", "-T", os.path.join(tmp_path, "missing.txt"), "--device", "-1"], capture_output=True, text=True)
    assert p.returncode != 0 and "cannot open trio file" in p.stdout + p.stderr
    # well-formed files fail only for want of a device: three fields, PED lines, blank lines and comments, skipped founders
    c, f, m = names[0], names[1], names[2]
    good = (f"{c} {f} {m}\n", f"{c}\t{f}\t{m}\r\n\n# a comment\n{names[3]} {names[4]} {names[5]}\n",
            f"fam1 {c} {f} {m} 1 2\nfam1 {f} 0 0 1 1\nfam1 {m} 0 0 2 1\n", f"fam1 {c} {f} {m} 1 2 extra columns\n{names[6]} {names[7]} {names[8]}\n")
    for k, text in enumerate(good):
        for more in ((), ("--per-trio",)):
            p = run(text, *more)
            out = p.stdout + p.stderr
            assert p.returncode != 0 and "device" in out.lower(), (k, out)
            assert "Sample not found" not in out and "trio file line" not in out and "no trios" not in out and "variantstore trios" not in out, (k, out)
            assert ("skipped 2 line(s)" in p.stderr) == (k == 2), (k, p.stderr)
    # a founder line that is all there is: nothing left
    p = run(f"fam1 {f} 0 0 1 1\nfam1 {m} {c} 0 2 1\n")
    assert p.returncode != 0 and "skipped 2 line(s)" in p.stderr and "no trios in" in p.stdout + p.stderr
    p = run("\n# nothing\n")
    assert p.returncode != 0 and "no trios in" in p.stdout + p.stderr
    # neither three fields nor six
    for text, line in ((f"{c} {f}\n", 1), (f"{c} {f} {m}\n{c} {f} {m} x\n", 2), (f"fam {c} {f} {m} 1\n", 1)):
        p = run(text)
        assert p.returncode != 0 and f"trio file line {line}" in p.stdout + p.stderr, text
    # unknown names, in either form; "ref" is no sample
    for text, who in ((f"{c} nobody-of-that-name {m}\n", "nobody-of-that-name"), (f"fam1 {c} {f} stranger 1 2\n", "stranger"), (f"{c} {f} ref\n", "ref")):
        p = run(text)
        assert p.returncode != 0 and f"Sample not found: {who}" in p.stdout + p.stderr, text
    # a trio that names a sample twice reaches the engine's own check
    p = run(f"{c} {f} {f}\n")
    assert p.returncode != 0 and "trio 0 " in p.stdout + p.stderr

"""Window statistics without a GPU (vs_query_window_stats on a handle opened host-only): the argument checks in the order the header
states them and VS_ERR_NO_DEVICE for a valid call; the reference (tests/window_stats_ref.py) on a hand-written text and against its
own brute force over the oracle's type-6 text of small random cohorts; the accessor's float64 formulas against the same formulas in
fractions.Fraction within the derived bounds; the command line's usage and -G file errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import window_stats_ref as ws
from helpers import oracle_texts, random_regions, write_random_cohort
from oracle.oracle import Oracle
from variantstore_amd import QueryResult, VariantStore, _lib, window_stats_derived
from variantstore_amd.api import VariantStoreError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS_ERR_NO_DEVICE, VS_ERR_ARG, VS_ERR_UNKNOWN_SAMPLE = -3, -5, -6


@pytest.fixture(scope="module")
def host_store(golden_dir):
    vs = VariantStore.from_vcf(os.path.join(golden_dir, "x.small.fa"), os.path.join(golden_dir, "x.small.vcf"), device=-1)
    yield vs
    vs.close()


def _call(vs, n=1, ids=(1,), gof=(0,), n_groups=1, names=None, n_ids=None, null_ids=False, null_gof=False, pairs=1):
    """vs_query_window_stats through ctypes: (code, message)."""
    lib = _lib.load()
    regions = (_lib.Region * max(n, 1))(*[_lib.Region(1, 100)] * max(n, 1))
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    b = np.ascontiguousarray(gof, dtype=np.uint32)
    pa = None if null_ids else a.ctypes.data_as(C.POINTER(C.c_uint32))
    pb = None if null_gof else b.ctypes.data_as(C.POINTER(C.c_uint32))
    pn = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names is not None else None
    h = C.c_void_p()
    rc = lib.vs_query_window_stats(vs._h, regions, n, pa, pb, len(a) if n_ids is None else n_ids, n_groups, pn, pairs, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.vs_last_error().decode()


def test_entry_points_are_declared():
    lib = _lib.load()
    for name in ("vs_query_window_stats", "vs_result_get_window_stats", "vs_result_window_stats_device"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert QueryResult.WINDOW_DTYPE.itemsize == 48 and QueryResult.WINDOW_PAIR_DTYPE.itemsize == 16
    assert QueryResult.WINDOW_DTYPE.names == ws.FIELDS and QueryResult.WINDOW_PAIR_DTYPE.names == ws.PAIR_FIELDS
    header = open(os.path.join(ROOT, "include", "variantstore_hip.h")).read()
    assert '"window_chunk"' in header and "vs_window_pair_stats" in header


def test_argument_errors_in_the_stated_order(host_store):
    vs = host_store
    ns = vs.info().num_samples
    assert ns == 2                                                          # x.small: "ref" and one sample, id 1
    # 1. the plain argument errors, as vs_query_group_counts
    assert _call(vs, n=0)[0] == VS_ERR_ARG
    assert "region" in _call(vs, n=0, pairs=2)[1]                           # before with_pairs
    assert _call(vs, null_ids=True, n_groups=2)[0] == VS_ERR_ARG            # NULL ids stand for the whole cohort with ONE group only
    assert _call(vs, null_gof=True)[0] == VS_ERR_ARG
    assert _call(vs, n_ids=0)[0] == VS_ERR_ARG
    assert _call(vs, n_groups=0)[0] == VS_ERR_ARG
    assert _call(vs, n_groups=65)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5,), n_groups=65)[0] == VS_ERR_ARG          # before the unknown sample
    # with_pairs: 0 or 1, right behind the range of n_groups and before the ids are looked at
    rc, msg = _call(vs, pairs=2)
    assert rc == VS_ERR_ARG and "with_pairs" in msg
    assert "with_pairs" in _call(vs, ids=(ns + 5,), pairs=7)[1]
    assert "with_pairs" in _call(vs, null_ids=True, pairs=2)[1]
    assert "groups" in _call(vs, n_groups=65, pairs=2)[1]
    # 2. a group out of range -- before an unknown sample
    assert _call(vs, ids=(1, 1), gof=(0, 2), n_groups=2)[0] == VS_ERR_ARG
    assert _call(vs, ids=(ns + 5, 1), gof=(0, 2), n_groups=2)[0] == VS_ERR_ARG
    # 3. "ref" or an id beyond the cohort -- before a conflicting membership
    assert _call(vs, ids=(0,), gof=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(ns,), gof=(0,))[0] == VS_ERR_UNKNOWN_SAMPLE
    assert _call(vs, ids=(1, 1, ns), gof=(0, 1, 0), n_groups=2)[0] == VS_ERR_UNKNOWN_SAMPLE
    # 4. a sample in two groups: the message names the sample and both groups
    rc, msg = _call(vs, ids=(1, 1, 1), gof=(1, 1, 4), n_groups=5)
    assert rc == VS_ERR_ARG and "sample id 1" in msg and "group 1" in msg and "group 4" in msg
    # a name with a tab or a newline
    assert _call(vs, names=["a\tb"])[0] == VS_ERR_ARG
    assert _call(vs, null_ids=True, names=["two\nlines"])[0] == VS_ERR_ARG


def test_valid_call_on_a_host_only_handle_has_no_device(host_store):
    vs = host_store
    for pairs in (0, 1):
        assert _call(vs, ids=(1, 1), gof=(63, 63), n_groups=64, pairs=pairs)[0] == VS_ERR_NO_DEVICE
        assert _call(vs, null_ids=True, null_gof=True, n_ids=0, pairs=pairs)[0] == VS_ERR_NO_DEVICE      # the whole cohort
        assert _call(vs, null_ids=True, n_ids=5, names=["all"], pairs=pairs)[0] == VS_ERR_NO_DEVICE      # (group_of and n_ids ignored)
    for kw in (dict(), dict(groups={"a": [1], "b": []}), dict(groups=[[1]], pairs=False)):
        with pytest.raises(VariantStoreError) as e:
            vs.window_stats([(1, 100)], **kw)
        assert e.value.code == VS_ERR_NO_DEVICE, kw
    with pytest.raises(VariantStoreError) as e:
        vs.window_stats([(1, 100)], [[1], [1]])
    assert e.value.code == VS_ERR_ARG
    with pytest.raises(VariantStoreError) as e:
        vs.window_stats([(1, 100)], {"a": ["nobody-of-that-name"]})
    assert e.value.code != VS_ERR_NO_DEVICE


HAND = ("Pos\tRef\tAlt\tSamples\n"
        "10\tA\tC\tS1(1|1) S2(0/1) S3(1/0) \n"
        "20\tG\tT\tS4(1|0) \n"
        "30\tC\tA\tS1(1|1) S2(1|1) \n"
        "30\tC\tG\tS3(1|1) S4(1/1) S9(1|1) \n"
        "40\tT\tG\t\n")
HAND_GROUPS = {"S1": 0, "S2": 0, "S3": 2, "S4": 2, "S9": 2}   # group 1 empty; S5 unlisted


def test_reference_on_a_hand_written_text():
    recs, prs, sizes = ws.region_records(HAND, HAND_GROUPS, 3)
    assert sizes == [2, 0, 3]
    # group 0 (N = 4): ac = 3, 0, 4, 0, 0; het = 1, 0, 0, 0, 0
    assert recs[0] == dict(rows=5, seg=1, singletons=0, doubletons=0, private=1, fixed=1, sum_ac=7, sum_ac2=25, obs_het=1)
    assert recs[1] == dict(rows=5, seg=0, singletons=0, doubletons=0, private=0, fixed=0, sum_ac=0, sum_ac2=0, obs_het=0)
    # group 2 (N = 6): ac = 1, 1, 0, 6, 0; het = 1, 1, 0, 0, 0
    assert recs[2] == dict(rows=5, seg=2, singletons=2, doubletons=0, private=2, fixed=1, sum_ac=8, sum_ac2=38, obs_het=2)
    assert [tuple(p.values()) for p in prs] == [(0, 1, 0), (3, 4, 2), (0, 2, 0)]   # pairs (0,1), (0,2), (1,2)
    got = ws.text(recs, prs, sizes, ["cases", "none", "controls"]).split("\n")
    assert got[0] + "\n" == ws.HEADER and got[1] == "cases\t2\t5\t1\t0\t0\t1\t1\t7\t25\t1" and got[4] + "\n" == ws.PAIR_HEADER
    assert got[6] == "cases\tcontrols\t3\t4\t2" and len(got) == 1 + 3 + 1 + 3 + 1
    assert ws.text(*ws.region_records(HAND, HAND_GROUPS, 3, pairs=False)).split("\n")[3] == "2\t3\t5\t2\t2\t0\t2\t1\t8\t38\t2"
    assert ws.PAIR_HEADER not in ws.text(*ws.region_records(HAND, HAND_GROUPS, 3, pairs=False))
    empty = ws.region_records("Pos\tRef\tAlt\tSamples\n", HAND_GROUPS, 3)
    assert all(v == 0 for r in empty[0] + empty[1] for v in r.values())
    # the brute force on the same text: group 0's copies at the first row are 1 1 0 1 -> 3 of 6 pairs differ
    members = [{"S1", "S2"}, set(), {"S3", "S4", "S9"}]
    assert ws.site_copies(HAND, members)[0] == [[1, 1, 0, 1], [], [1, 0, 0, 0, 0, 0]]
    pi, dxy, fst = ws.brute_force(HAND, members)
    assert pi[0] == ws.exact_pi(recs[0], 2) == ws.Fraction(1, 2) and pi[1] is None and pi[2] == ws.exact_pi(recs[2], 3)
    assert dxy[0] is None and dxy[2] is None and dxy[1] == ws.exact_dxy(recs[0], recs[2], prs[1], 2, 3)


@pytest.mark.parametrize("seed", [811, 812])
def test_formulas_against_brute_force_and_fractions(seed, tmp_path):
    """9 samples, 150 rows: the N sum_ac - sum_ac2 algebra against counted pairs, exactly; then the accessor's float64 values
    against the exact ones within the bounds window_stats_ref derives."""
    fasta, vcf, names = write_random_cohort(str(tmp_path), seed, ref_len=3000, n_rows=150, n_samples=9, p_multi=0.3, p_same=0.2,
                                            unphased_p=0.3, carrier_p=0.5 if seed % 2 else 0.2, haploid_p=0.1)
    vs = VariantStore.from_vcf(fasta, vcf, device=-1)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    vs.close()
    orc = Oracle(plain)
    rng = np.random.default_rng(seed)
    regions = random_regions(rng, 3000, 25, max_len=900)
    want = [(r, t) for r, (n, _e, t) in zip(regions, oracle_texts(orc, regions)) if n >= 0]
    groupings = [[names], [names[:1], names[1:]], [names[:4], [], names[4:8]], [[n] for n in names], [names[:2], names[2:5], names[5:]]]
    defined = 0
    for members in groupings:
        group_of = {nm: g for g, m in enumerate(members) for nm in m}
        all_recs, all_prs = [], []
        for _region, text in want:
            recs, prs, sizes = ws.region_records(text, group_of, len(members))
            pi, dxy, fst = ws.brute_force(text, [set(m) for m in members])
            for g in range(len(members)):
                assert pi[g] == ws.exact_pi(recs[g], sizes[g]), (g, text)
            for p, (g, h) in enumerate(ws.pair_list(len(members))):
                assert dxy[p] == ws.exact_dxy(recs[g], recs[h], prs[p], sizes[g], sizes[h])
                assert fst[p] == ws.exact_fst(ws.exact_pi(recs[g], sizes[g]), ws.exact_pi(recs[h], sizes[h]), dxy[p])[0]
                defined += fst[p] is not None
            all_recs.append(recs); all_prs.append(prs)
        stats, pairs = ws.arrays(all_recs, all_prs, QueryResult.WINDOW_DTYPE, QueryResult.WINDOW_PAIR_DTYPE)
        got = window_stats_derived(stats, pairs, sizes, lengths=[y - x + 1 if y >= x else 1 for (x, y), _t in want])
        ws.check_derived(got, all_recs, all_prs, sizes)
        assert got["pair_index"].tolist() == [list(p) for p in ws.pair_list(len(members))]
        assert got["pi_per_bp"].shape == got["pi"].shape
        if len(members) == 1:
            assert np.isfinite(got["tajima_d"]).any() and got["dxy"].shape == (len(want), 0)
        if len(members) == 9:   # one sample a group: N = 2, pi defined, Tajima's D not
            assert np.isnan(got["tajima_d"]).all() and np.isfinite(got["pi"]).all()
    assert defined > 50


def test_undefined_quantities_are_nan():
    stats = np.zeros((2, 3), QueryResult.WINDOW_DTYPE)
    pairs = np.zeros((2, 3), QueryResult.WINDOW_PAIR_DTYPE)
    stats["rows"][1] = 4
    stats["sum_ac"][1, 0], stats["sum_ac2"][1, 0], stats["seg"][1, 0] = 6, 14, 3
    got = window_stats_derived(stats, pairs, [3, 0, 1])
    assert np.isnan(got["pi"][:, 1]).all() and np.isnan(got["theta_w"][:, 1]).all() and np.isnan(got["het_obs"][:, 1]).all()
    assert got["pi"][0, 0] == 0.0 and math.isnan(got["tajima_d"][0, 0]) and math.isnan(got["het_obs"][0, 0])   # no site, no row
    assert got["pi"][1, 0] == 2.0 * (6 * 6 - 14) / 30 and math.isfinite(got["tajima_d"][1, 0]) and got["het_obs"][1, 0] == 0.0
    assert math.isnan(got["tajima_d"][1, 2]) and got["pi"][1, 2] == 0.0                                        # N = 2
    assert np.isnan(got["dxy"][:, 0]).all() and np.isnan(got["dxy"][:, 2]).all()                              # an empty group
    assert got["dxy"][0, 1] == 0.0 and got["dxy"][1, 1] == 2 * 6 / 12
    fst = got["fst_hudson"]
    assert np.isnan(fst[:, 0]).all() and np.isnan(fst[:, 2]).all() and math.isnan(fst[0, 1])                  # ... and dxy = 0
    assert fst[1, 1] == 1.0 - ((got["pi"][1, 0] + 0.0) / 2.0) / 1.0
    with pytest.raises(ValueError):
        window_stats_derived(stats, pairs, [3, 0, 1], lengths=[1, 2, 3])


def test_cli_usage_and_group_file_errors(golden_dir, tmp_path):
    exe = os.path.join(ROOT, "variantstore_amd", "bin", "variantstore")
    p = subprocess.run([exe, "windows"], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore windows " in p.stdout
    prefix = os.path.join(tmp_path, "idx")
    os.makedirs(prefix)
    subprocess.run([exe, "construct", "-r", os.path.join(golden_dir, "x.small.fa"), "-v", os.path.join(golden_dir, "x.small.vcf"), "-p", prefix],
                   check=True, capture_output=True)
    p = subprocess.run([exe, "windows", "-p", prefix], capture_output=True, text=True)
    assert p.returncode != 0 and "variantstore windows " in p.stdout
    p = subprocess.run([exe, "windows", "-p", prefix, "-r", "1:100", "--nprocs", "2"], capture_output=True, text=True)
    assert p.returncode != 0 and "unknown option --nprocs" in p.stdout + p.stderr
    host = VariantStore.open(prefix, device=-1)
    name = host.sample_name(1)
    host.close()
    gfile = os.path.join(tmp_path, "groups.txt")

    def run(text, cmd="windows", *more):
        with open(gfile, "w") as f:
            f.write(text)
        r = subprocess.run([exe, cmd, "-p", prefix, "-r", "1:100", "-G", gfile, "--device", "-1", *more], capture_output=True, text=True)
        assert r.returncode != 0
        return r.stdout + r.stderr

    for text, said in ((f"{name}\ta\nnobody-of-that-name\tb\n", "Sample not found: nobody-of-that-name"), (f"{name}\ta\n{name}\tb\n", "two groups"),
                       (f"{name}\n", "no group on the line"), ("\n\n", "no sample-group pairs"),
                       ("".join(f"{name}\tg{i}\n" for i in range(65)), "two groups")):
        assert said in run(text) and said in run(text, "groups"), said                # the -G file's errors follow `groups`
    os.remove(gfile)
    r = subprocess.run([exe, "windows", "-p", prefix, "-r", "1:100", "-G", gfile, "--device", "-1"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open group file" in r.stdout + r.stderr
    # a valid call on a host-only handle: the query's refusal, with and without the file and the switches
    for more in ((), ("--no-pairs",), ("--derived",)):
        assert "windows: no GPU device" in run(f"{name}\ta\n", "windows", *more)
    r = subprocess.run([exe, "windows", "-p", prefix, "-r", "1:100", "--device", "-1", "--derived"], capture_output=True, text=True)
    assert r.returncode != 0 and "windows: no GPU device" in r.stdout + r.stderr

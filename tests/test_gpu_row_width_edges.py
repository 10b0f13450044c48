"""Parity at the class-row widths where the carrier expansion changes shape: wpc = ceil(info().num_samples / 64) of 63 (the widest
non-WIDE row: 32-bit slices, the zero word behind the row, the least LDS slack) and 64 (the only width at which the WIDE
instantiation takes its staged medium and dense paths instead of the generic one), each with a last row word of one bit and a full
one.  Every check is text-exact against the oracle, through the helpers of the other GPU test files; the preconditions that make a
case prove anything are asserted from what the oracle-checked answer reports (carrier counts, arena offsets, carrier ids).

Two cohorts per width:
  spread     VariantStore.synthetic with af_exponent 3.5: listed, medium and dense variants together.  (3.5, not 2.5: at these
             widths the rarest allele of 2.5 still has ~26 carriers, and VS_LIST_MAX=0 is to send rows of 1..8 carriers through the
             row paths.)
  saturated  VCF text of helpers.write_saturated_cohort (seed 4400 + S): the synthetic generator caps an allele's frequency at 0.5 -- at most ~76 % of the
             samples carry a variant -- so rows carried by 75 - 99 % of the samples, and every eighth row by all but 0..5 of them, are
             written out and opened with from_vcf."""
import os

import numpy as np
import pytest

from helpers import write_saturated_cohort
from oracle.oracle import Oracle
from test_gpu_allele_counts import _check_texts
from test_gpu_genotype_matrix import _check as _check_matrix, _parse as _parse_matrix
from test_gpu_ld_band import _check_full
from test_gpu_parity import _compare_t4, _compare_t6
from test_gpu_sample_burden import _check as _check_burden, _parse as _parse_burden
from variantstore_amd import VariantStore

pytestmark = pytest.mark.gpu

WIDTHS = [3968, 4031, 4032, 4095]       # wpc 63 / 63 / 64 / 64; last row word: 1 bit / full / 1 bit / full
SPREAD_SEED = {3968: 611, 4031: 612, 4032: 613, 4095: 614}
SPREAD_KW = dict(ref_length=60_000, num_variants=300, first_pos=100, frac_ins=0.06, frac_del=0.06, frac_multi=0.03, max_indel=4,
                 af_exponent=3.5)


class _Memo:
    """The oracle with every answer kept: a cohort's checks share their regions, the reference is computed once."""

    def __init__(self, orc):
        self._orc, self._t6, self._t4 = orc, {}, {}

    def get_var_in_ref(self, x, y):
        if (x, y) not in self._t6:
            self._t6[(x, y)] = self._orc.get_var_in_ref(x, y)
        return self._t6[(x, y)]

    def get_sample_var_in_ref(self, x, y, sample):
        if (x, y, sample) not in self._t4:
            self._t4[(x, y, sample)] = self._orc.get_sample_var_in_ref(x, y, sample)
        return self._t4[(x, y, sample)]


def _open(n_samples, profile, tmp_path):
    """(store, memoised oracle) of one cohort, after the asserts every case makes about its width."""
    if profile == "spread":
        vs = VariantStore.synthetic(device=0, num_samples=n_samples, seed=SPREAD_SEED[n_samples], **SPREAD_KW)
    else:
        fasta, vcf = write_saturated_cohort(str(tmp_path), n_samples, 4400 + n_samples)
        vs = VariantStore.from_vcf(fasta, vcf, device=0)
    info = vs.info()
    assert info.num_samples - 1 == n_samples and info.use_bit_vector
    assert (info.num_samples + 63) // 64 == (n_samples + 1 + 63) // 64 == (63 if n_samples <= 4031 else 64)
    plain = os.path.join(tmp_path, "plain.bin")
    vs.export_plain(plain)
    return vs, _Memo(Oracle(plain))


def _batch(vs, profile, seed):
    """70 sorted overlapping regions (more than 64: the throughput path) over the whole reference."""
    rng = np.random.default_rng(seed)
    L, span = vs.info().ref_length, 1500 if profile == "spread" else 420
    starts = np.sort(rng.integers(1, L - span, size=70))
    return [(int(s), int(s) + int(rng.integers(span // 2, span))) for s in starts]


def _edge_samples(n_samples):
    """Ids 1, 63 and 64 (the first word's end, the second's start), the first sample of the last row word, the last sample."""
    wpc = (n_samples + 1 + 63) // 64
    return sorted({1, 63, 64, (wpc - 1) * 64, n_samples})


def _unique_rows(vs, regions):
    """What the (oracle-checked) answer to `regions` reports about its table rows, each site once: (car_count, arena offset, the
    rows' carrier id arrays)."""
    res = vs.get_var_in_ref(regions)
    assert res.layout()[4], "a sorted batch shares rows and carrier lists"
    raw = res.raw(with_carriers=False)
    cnt = (raw["rows"]["count_flags"] & 0x7FFFFFFF).astype(np.int64)
    cnt[(raw["rows"]["count_flags"] >> 31) != 0] = 0
    begin = raw["rows"]["car_begin"].astype(np.int64)
    view = res.view(with_carriers=True)
    seen, ids = set(), []
    for a in range(view["pos"].shape[0]):
        key = (int(view["pos"][a]), int(view["alt_off"][a]), int(view["alt_len"][a]), int(view["car_count"][a]))
        if key not in seen:
            seen.add(key)
            b = int(view["car_begin"][a])
            ids.append(view["carriers"][b:b + int(view["car_count"][a])] & 0x1FFFFFFF)
    res.close()
    return cnt, begin, ids


@pytest.mark.parametrize("list_max", [None, 64, 0])
@pytest.mark.parametrize("profile", ["spread", "saturated"])
@pytest.mark.parametrize("n_samples", WIDTHS)
def test_type6_and_type4_at_the_boundary_widths(n_samples, profile, list_max, tmp_path, monkeypatch):
    """Query types 6 and 4 through every form of the expansion: the shared path (k_fill_sites2: sorted, shuffled), private rows
    (k_fill_carriers), the latency launches of 8 and of 64 region slots (k_query_small), resident lists, and the event-bitmap walk
    of type 4 for the samples at the row words' edges."""
    if list_max is None:
        monkeypatch.delenv("VS_LIST_MAX", raising=False)
    else:
        monkeypatch.setenv("VS_LIST_MAX", str(list_max))
    vs, orc = _open(n_samples, profile, tmp_path)
    list_max = 640 if list_max is None else list_max
    assert vs.info().list_max == list_max
    wide = n_samples > 4031
    regions = _batch(vs, profile, n_samples)
    rng = np.random.default_rng(n_samples + list_max)

    assert _compare_t6(vs, orc, regions) == len(regions)                                   # shared rows and lists
    assert _compare_t6(vs, orc, [regions[i] for i in rng.permutation(len(regions))]) == len(regions)
    vs.set_option("share_lists", 0)
    assert _compare_t6(vs, orc, regions) == len(regions)                                   # private rows
    vs.set_option("share_lists", 1)
    vs.set_option("latency_server", 0)                                                      # one launch per small batch
    assert _compare_t6(vs, orc, regions[:3]) == 3                                          # 8 region slots
    assert _compare_t6(vs, orc, regions[10:30]) == 20                                      # 64 region slots
    vs.set_option("latency_server", 1)
    plain_res = vs.get_var_in_ref(regions)
    digest, totals = plain_res.digest(), plain_res.totals()
    plain_res.close()
    vs.set_option("resident_lists", 1)
    res = vs.get_var_in_ref(regions)
    assert res.layout()[2] == 0 and (res.digest(), res.totals()) == (digest, totals), "resident carrier lists change the answers"
    res.close()
    assert _compare_t6(vs, orc, regions) == len(regions)
    vs.set_option("resident_lists", 0)
    picks = [regions[i] for i in range(0, len(regions), 6)]                                # 12 regions
    for sid in _edge_samples(n_samples):
        assert _compare_t4(vs, orc, picks, vs.sample_name(sid)) == len(picks), sid

    # ---- what this cohort sent through the kernel: conditions on the inputs, from the answer checked above
    cnt, begin, ids = _unique_rows(vs, regions)
    row_path = cnt > list_max
    if wide and profile == "spread" and list_max == 64:
        assert ((cnt > 64) & (cnt <= 640)).sum() > 20 and (cnt > 640).sum() > 20          # WIDE medium and WIDE dense
    if wide:
        dense = row_path & (cnt > 640)
        assert (begin[dense] % 256 != 0).any(), "no dense row starts inside a 1 KiB block of the arena"
        assert (cnt[dense] > 512).any()                                                    # at least two 1 KiB blocks
    if n_samples == 4095 and profile == "saturated":
        assert (cnt >= 4090).sum() >= 5                                                    # candidates for nshift + cnt > 4096 (not staged)
        assert ((cnt > 2048) & (cnt < 4060)).sum() >= 20                                   # staged, both nibble loads
    if n_samples == 4031:
        if profile == "saturated":
            assert (cnt > 2100).sum() >= 20                                                # the list does not fit: rebase with o != 0
        on_rows = [i for i in ids if i.shape[0] > list_max]
        assert any((i == 4031).any() for i in on_rows), "no row-path row is carried by the last sample"
        if profile == "saturated" or list_max == 0:                                        # (spread: only among the rare alleles VS_LIST_MAX=0 adds)
            assert any(not (i >= 2016).any() for i in on_rows), "no row whose second round is empty"
    if list_max == 0 and profile == "spread":
        assert ((cnt >= 1) & (cnt <= 7)).any() and (cnt == 8).any()                        # an incomplete and a complete single group
    vs.close()


@pytest.mark.parametrize("n_samples", [4031, 4032, 4095])
def test_consumers_at_the_boundary_widths(n_samples, tmp_path, monkeypatch):
    """The kernels that read the same image and switch on the same width -- allele counts, per-sample burden, the genotype matrix,
    banded LD -- once each on the spread cohort with VS_LIST_MAX=64, through the references of their own test files."""
    monkeypatch.setenv("VS_LIST_MAX", "64")
    vs, orc = _open(n_samples, "spread", tmp_path)
    regions = _batch(vs, "spread", n_samples)
    cnt, _begin, _ids = _unique_rows(vs, regions)
    assert (cnt > 64).sum() > 20 and (cnt <= 64).sum() > 20, "both storage forms"
    rng = np.random.default_rng(n_samples)
    subset = sorted({1, 63, 64, n_samples - 1, n_samples} | {int(i) for i in rng.choice(np.arange(1, n_samples + 1), size=40, replace=False)})
    names = {vs.sample_name(i) for i in subset}
    want = [orc.get_var_in_ref(x, y) for x, y in regions]
    assert _check_texts(vs, regions, want) == len(regions)
    assert _check_texts(vs, regions, want, subset, names) == len(regions)
    parsed, valid = _parse_burden(orc, regions)
    _check_burden(vs, regions, parsed, valid, subset, texts=True)
    if n_samples == 4095:
        _check_burden(vs, regions, parsed, valid, None)
    parsed, valid = _parse_matrix(orc, regions)
    got = _check_matrix(vs, regions, parsed, valid, None)
    assert got["cells"][:, -1].any(), "the last column is set nowhere"
    assert got["row_pitch"] == (n_samples + 15) // 16 * 16                                 # 4032, 4032, 4096
    m = _check_full(vs, regions, None, (16, 100), n_samples)                               # the k loop's tail at that pitch
    assert m["cells"].shape == (got["cells"].shape[0], n_samples)
    vs.close()

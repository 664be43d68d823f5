"""The flat inner-product main pass at padded dim 128, k <= 8, in both workgroup
forms: 256 queries (4 waves) and 512 queries (8 waves, the plan's choice from
4096 queries on), forced either way with the NRK_SCREEN_WAVES test hook.  Every
case is checked against the oracle: ids and fp32 distances bit-equal."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

NQ_MAX = 1100


@functools.lru_cache(maxsize=None)
def _data(n, d):
    rng = np.random.default_rng(1000 * d + n % 13)
    c = rng.standard_normal((64, d)).astype(np.float32)
    xb = (c[rng.integers(0, 64, n)] + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    xq = (c[rng.integers(0, 64, NQ_MAX)] + 0.35 * rng.standard_normal((NQ_MAX, d))).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xq, xb


@functools.lru_cache(maxsize=None)
def _index(n, d, metric):
    from newsrecommend_amd import faiss as nf

    idx = nf.IndexFlat(d, metric)
    idx.add(_data(n, d)[1])
    return idx


@functools.lru_cache(maxsize=None)
def _oracle(n, d, k, metric):
    """The oracle's answer for all NQ_MAX queries (a case with fewer takes the
    first rows: queries are independent)."""
    xq, xb = _data(n, d)
    Do, Io, _ = ko.exact_search(xq, xb, k, metric)
    return Do, Io


def _planned(nq, nb, d, k, metric):
    from newsrecommend_amd import _lib

    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().nrk_knn_flat_main_pass(nq, nb, d, k, metric, buf, 256), "knn_flat_main_pass")
    return buf.value.decode()


@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("nq", [300, 512, 513, 1100])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("d", [128, 100])
@pytest.mark.parametrize("n", [60_001, 70_003])
def test_inner_product_both_forms(gpu, monkeypatch, n, d, k, nq, waves):
    """Chunks ending in partial tiles, d padded to 128, and query counts below
    one 512-query tile, exactly one, one row over, and a partial third."""
    monkeypatch.setenv("NRK_SCREEN_WAVES", waves)
    name = _planned(nq, n, d, k, ko.METRIC_IP)
    assert f"{waves} waves" in name and "screen16_kernel" in name, name
    D, I = _index(n, d, ko.METRIC_IP).search(_data(n, d)[0][:nq], k)
    Do, Io = _oracle(n, d, k, ko.METRIC_IP)
    np.testing.assert_array_equal(I, Io[:nq])
    np.testing.assert_array_equal(D, Do[:nq])


def test_plan_takes_the_8_wave_form_from_4096_queries(gpu, monkeypatch):
    monkeypatch.delenv("NRK_SCREEN_WAVES", raising=False)
    assert "8 waves" in _planned(4096, 1_000_000, 128, 5, ko.METRIC_IP)
    assert "8 waves" in _planned(5000, 1_000_000, 100, 8, ko.METRIC_IP)
    assert "4 waves" in _planned(4095, 1_000_000, 128, 5, ko.METRIC_IP)
    assert "4 waves" in _planned(4096, 1_000_000, 128, 5, ko.METRIC_L2)
    assert "4 waves" in _planned(4096, 1_000_000, 128, 10, ko.METRIC_IP)
    assert "4 waves" in _planned(4096, 1_000_000, 64, 5, ko.METRIC_IP)


@pytest.mark.parametrize("waves", ["4", "8"])
def test_duplicate_blocks_across_a_chunk_boundary(gpu, monkeypatch, waves):
    """Blocks of identical rows across a chunk boundary (60,001 rows and 600
    queries plan 1024-row chunks in both forms) and inside one 32-item sub-tile,
    searched with those rows: the lower ids win."""
    from newsrecommend_amd import faiss as nf

    monkeypatch.setenv("NRK_SCREEN_WAVES", waves)
    xq, xb = (a.copy() for a in _data(60_001, 128))
    xq = xq[:600]
    blocks = [(1018, 1031), (2047, 2049), (30_720 - 3, 30_720 + 9), (5000, 5012)]
    for i, (lo, hi) in enumerate(blocks):
        xb[lo:hi] = xb[lo] * np.float32(3.0)  # the row's own copies are its best inner products
        xq[i] = xb[lo]
        xq[512 + i] = xb[lo]
    assert f"{waves} waves" in _planned(600, 60_001, 128, 8, ko.METRIC_IP)
    idx = nf.IndexFlat(128, ko.METRIC_IP)
    idx.add(xb)
    D, I = idx.search(xq, 8)
    Do, Io, _ = ko.exact_search(xq, xb, 8, ko.METRIC_IP)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    for i, (lo, hi) in enumerate(blocks):
        want = list(range(lo, min(hi, lo + 8)))
        assert I[i, :len(want)].tolist() == want
        assert I[512 + i, :len(want)].tolist() == want


@pytest.mark.parametrize("nq", [300, 1100])
@pytest.mark.parametrize("d", [128, 100])
@pytest.mark.parametrize("n", [60_001, 70_003])
def test_l2_keeps_its_form_under_the_hook(gpu, monkeypatch, n, d, nq):
    monkeypatch.setenv("NRK_SCREEN_WAVES", "8")
    assert "4 waves" in _planned(nq, n, d, 5, ko.METRIC_L2)
    D, I = _index(n, d, ko.METRIC_L2).search(_data(n, d)[0][:nq], 5)
    Do, Io = _oracle(n, d, 5, ko.METRIC_L2)
    np.testing.assert_array_equal(I, Io[:nq])
    np.testing.assert_array_equal(D, Do[:nq])

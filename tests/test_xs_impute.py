"""Factor imputation of missing characteristics (data/transforms.py): the numpy definitions on
hand-checkable cases, the prepared directory through the loader, and the quality on a planted panel."""
import os

import numpy as np
import pytest

import impute_cases as ic
import rank_cases as rc
from deeplearninginassetpricing_paperreplication_amd.data import transforms as tr
from deeplearninginassetpricing_paperreplication_amd.data.dataset import MISSING_VALUE, load_splits

NAN = np.float32(np.nan)

# Quality on the planted panel (impute_cases.PLANTED: 3 x 300 x 46, Kt = 4, K = 6, seed 11, 15 % holes):
# the numpy definition gave the ratio 0.7614811 when this test was written (the median fill is 1);
# the bound is the midpoint between that and 1.
QUALITY_MEASURED = 0.7614811
QUALITY_BOUND = (QUALITY_MEASURED + 1.0) / 2


def f32(a):
    return np.asarray(a, dtype=np.float32)


def test_moments_by_hand():
    y = f32([[[0.5, NAN], [0.25, 0.125], [NAN, -0.5], [7.0, 7.0]]])            # the last row is dead
    rowok = np.array([[True, True, True, False]])
    S, C = tr.characteristic_moments_numpy(y, rowok)
    assert S.dtype == np.float64 and C.dtype == np.int32 and S.shape == C.shape == (1, 2, 2)
    assert np.array_equal(C[0], [[2, 1], [1, 2]])
    assert np.array_equal(S[0], [[0.25 + 0.0625, 0.03125], [0.03125, 0.015625 + 0.25]])


def test_single_characteristic():
    y = f32([[[0.25], [NAN], [-0.5]]])
    rowok = np.ones((1, 3), dtype=bool)
    S, C = tr.characteristic_moments_numpy(y, rowok)
    assert S[0, 0, 0] == 0.3125 and C[0, 0, 0] == 2
    lam, explained = tr.xs_loadings(S, C, 6)                                    # K > F
    assert lam.shape == (1, 1, 1) and lam.dtype == np.float32 and lam[0, 0, 0] == 1.0 and explained[0] == 1.0
    out = tr.xs_fill_numpy(y, rowok, lam, 0.01)
    assert out[0, 1, 0] == 0.0                                                   # no observed entry: b = 0
    assert np.array_equal(rc.bits(out[0, [0, 2]]), rc.bits(y[0, [0, 2]]))


def test_columns_never_observed_together():
    y = f32([[[0.5, NAN], [-0.5, NAN], [NAN, 0.25], [NAN, -0.25]]])
    rowok = np.ones((1, 4), dtype=bool)
    S, C = tr.characteristic_moments_numpy(y, rowok)
    assert C[0, 0, 1] == C[0, 1, 0] == 0 and S[0, 0, 1] == 0.0
    lam, explained = tr.xs_loadings(S, C, 1)                                    # Sig = diag(0.25, 0.0625)
    assert np.array_equal(lam[0], f32([[1.0], [0.0]])) and explained[0] == 0.8
    out = tr.xs_fill_numpy(y, rowok, lam, 0.01)
    assert np.all(out[0, :, :][y[0] != y[0]] == 0.0)                            # column 1 loads on nothing


def test_period_without_kept_rows_and_garbage_in_dead_rows():
    rng = np.random.default_rng(0)
    y = (rng.random((2, 6, 3)) - 0.5).astype(np.float32)
    y[0, 1, 2] = NAN
    y[0, 4, 0] = NAN
    rowok = np.ones((2, 6), dtype=bool)
    rowok[1] = False
    rowok[0, 5] = False
    dirty = y.copy()
    dirty[1] = f32([np.nan, np.inf, -1e30])
    dirty[0, 5] = f32([np.inf, np.nan, 3.0])
    S, C = tr.characteristic_moments_numpy(y, rowok)
    S2, C2 = tr.characteristic_moments_numpy(dirty, rowok)
    assert np.array_equal(S, S2) and np.array_equal(C, C2)
    assert not C[1].any() and not S[1].any()
    lam, explained = tr.xs_loadings(S, C, 2)
    assert not lam[1].any() and explained[1] == 0.0 and 0.0 < explained[0] <= 1.0
    out = tr.xs_fill_numpy(dirty, rowok, lam, 0.01)
    keep = np.ones(y.shape, dtype=bool)
    keep[0, 1, 2] = keep[0, 4, 0] = False
    assert np.array_equal(rc.bits(out)[keep], rc.bits(dirty)[keep])              # dead rows keep their bits
    assert np.array_equal(rc.bits(out[0, :5]), rc.bits(tr.xs_fill_numpy(y, rowok, lam, 0.01)[0, :5]))


def test_row_with_one_observed_entry():
    lam = f32([[[0.6], [0.8]]])
    y = f32([[[0.25, NAN], [0.125, -0.375]]])
    rowok = np.ones((1, 2), dtype=bool)
    out = tr.xs_fill_numpy(y, rowok, lam, 0.01)
    l0, l1 = np.float64(np.float32(0.6)), np.float64(np.float32(0.8))
    want = np.float32(l1 * (l0 * 0.25) / (0.01 + l0 * l0))
    assert out[0, 0, 1] == want and out[0, 0, 0] == 0.25
    assert np.array_equal(rc.bits(out[0, 1]), rc.bits(y[0, 1]))                  # fully observed: untouched
    big = tr.xs_fill_numpy(f32([[[0.5, NAN]]]), np.ones((1, 1), dtype=bool), f32([[[0.1], [3.0]]]), 0.01)
    assert big[0, 0, 1] == 0.5                                                   # clipped


def test_fully_observed_panel_keeps_every_bit():
    y, rowok = ic.ranked_case((3, 65, 5))
    full = np.where(y == y, y, np.float32(0.125)).astype(np.float32)
    lam, _ = tr.xs_loadings(*tr.characteristic_moments_numpy(full, rowok), 3)
    assert np.array_equal(rc.bits(tr.xs_fill_numpy(full, rowok, lam, 0.01)), rc.bits(full))


def test_gamma_must_be_positive():
    y, rowok, lam, _ = ic.fill_case((3, 65, 5), 1)
    for g in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            tr.xs_fill_numpy(y, rowok, lam, g)
        with pytest.raises(ValueError):
            tr.xs_fill(y, rowok, lam, g, device="cpu")


def test_loadings():
    S, C = ic.moments_case((3, 65, 46))
    lam, explained = tr.xs_loadings(S, C, 6)
    assert lam.shape == (3, 46, 6) and lam.dtype == np.float32 and explained.shape == (3,)
    assert not lam[2].any()                                                      # the dead last period
    for t in range(2):
        l = lam[t].astype(np.float64)
        assert np.allclose(l.T @ l, np.eye(6), atol=1e-6)
        big = np.abs(l).argmax(axis=0)
        assert np.all(l[big, np.arange(6)] > 0)
        sig = np.where(C[t] > 0, S[t] / np.maximum(C[t], 1), 0.0)
        top = np.sort(np.linalg.eigvalsh(sig))[::-1][:6]
        assert np.allclose(np.einsum("fk,fg,gk->k", l, sig, l), top, atol=1e-6)  # the top six, in descending order
    assert tr.xs_loadings(S, C, 100)[0].shape == (3, 46, 46)


def test_flipping_an_eigenvector_changes_no_output_bit():
    y, rowok, lam, want = ic.fill_case((2, 300, 46), 6)
    flipped = lam.copy()
    flipped[:, :, 1] = -flipped[:, :, 1]
    flipped[0, :, 4] = -flipped[0, :, 4]
    assert np.array_equal(rc.bits(tr.xs_fill_numpy(y, rowok, flipped, ic.GAMMA)), rc.bits(want))


def test_dispatch_on_the_cpu_is_the_definition():
    y, rowok, lam, want = ic.fill_case((3, 65, 5), 6)
    S, C = tr.characteristic_moments(y, rowok, device="cpu")
    assert np.array_equal(S, ic.moments_case((3, 65, 5))[0]) and np.array_equal(C, ic.moments_case((3, 65, 5))[1])
    assert np.array_equal(rc.bits(tr.xs_fill(y, rowok, lam, ic.GAMMA, device="cpu")), rc.bits(want))
    buf = y.copy()
    assert tr.xs_fill(buf, rowok, lam, ic.GAMMA, out=buf, device="cpu") is buf   # in place
    assert np.array_equal(rc.bits(buf), rc.bits(want))


def test_row_filter_treats_xs_as_median():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 30, 6)).astype(np.float32)
    x[rng.random(x.shape) < 0.3] = np.float32(MISSING_VALUE)
    ret = rng.standard_normal((2, 30)).astype(np.float32)
    ret[0, 3] = np.float32(MISSING_VALUE)
    assert tr.IMPUTE == ("none", "median", "xs")
    for k in (0, 1, 4, 6):
        assert np.array_equal(tr.row_filter(ret, x, "xs", k), tr.row_filter(ret, x, "median", k))


@pytest.fixture(scope="module")
def prepared(shipped_data, tmp_path_factory):
    """The raw directory prepared twice on the CPU: median and xs at the same min_characteristics."""
    root = tmp_path_factory.mktemp("xs_prepared")
    raw = rc.make_raw_dir(shipped_data, str(root / "raw"))
    reports = {}
    for impute in ("median", "xs"):
        reports[impute] = tr.main(["--input_dir", raw, "--output_dir", str(root / impute), "--impute", impute,
                                   "--min_characteristics", "23", "--impute_factors", "6", "--impute_ridge", "0.01",
                                   "--device", "cpu"])
    return root, reports


def test_prepared_directory_loads_with_the_mask_of_median(prepared):
    root, reports = prepared
    for s, a, b in zip(("train", "valid", "test"), load_splits(str(root / "xs")), load_splits(str(root / "median"))):
        assert np.array_equal(a.mask, b.mask) and a.mask.any()
        assert np.array_equal(rc.bits(a.returns), rc.bits(b.returns))
        assert np.all(np.abs(a.individual_features) <= 0.5)
        rx, rm = reports["xs"][s], reports["median"][s]
        assert rx["impute"] == "xs" and rx["impute_factors"] == 6 and rx["impute_ridge"] == 0.01
        assert 0.0 < rx["explained"] <= 1.0
        assert not {"impute_factors", "impute_ridge", "imputed_entries", "explained"} & set(rm)
        assert {k: v for k, v in rx.items() if k in rm and k not in ("impute", "seconds")} == \
               {k: v for k, v in rm.items() if k not in ("impute", "seconds")}


def test_bytes_differ_from_median_exactly_at_the_holes_of_kept_rows(prepared):
    root, reports = prepared
    for s in ("train", "valid", "test"):
        with np.load(os.path.join(root, "raw", "char", f"Char_{s}.npz")) as z:
            raw = z["data"]
        with np.load(os.path.join(root, "xs", "char", f"Char_{s}.npz")) as z:
            xs = z["data"]
        with np.load(os.path.join(root, "median", "char", f"Char_{s}.npz")) as z:
            med = z["data"]
        rowok = tr.row_filter(raw[:, :, 0], raw[:, :, 1:], "xs", 23)
        holes = np.zeros(raw.shape, dtype=bool)
        holes[:, :, 1:] = rowok[:, :, None] & ~(raw[:, :, 1:] > tr.THR)
        assert holes.any() and xs.dtype == np.float32
        assert np.array_equal(rc.bits(xs) != rc.bits(med), holes)
        assert np.all(med[holes] == 0.0) and not np.isnan(xs).any()
        assert reports["xs"][s]["imputed_entries"] == holes.sum()


def test_quality_on_the_planted_panel(capsys):
    data, full_ranks, gone = ic.planted_data()
    out, rep = tr.prepare_split(data, "xs", 1, "cpu", impute_factors=ic.PLANTED["K"], impute_ridge=ic.GAMMA)
    ratio = ic.quality_ratio(out[:, :, 1:], full_ranks, gone)
    with capsys.disabled():
        print(f"\n[xs quality] imputed RMSE / median-fill RMSE = {ratio:.7f} (bound {QUALITY_BOUND:.7f})")
    assert rep["imputed_entries"] == gone.sum() and 0.0 < rep["explained"] < 1.0
    med, _ = tr.prepare_split(data, "median", 1, "cpu")
    assert ic.quality_ratio(med[:, :, 1:], full_ranks, gone) == 1.0
    assert ratio <= QUALITY_BOUND

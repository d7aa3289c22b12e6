"""Cross-sectional rank transform (data/transforms.py): the definition against a brute-force count,
its exact properties, the row rule, and a raw directory through ``prepare_data_dir``, the
unmodified loader and a short CPU training run."""
import filecmp
import json
import os

import numpy as np
import pytest

import golden_cases as gc
import rank_cases as rc
from deeplearninginassetpricing_paperreplication_amd.data import transforms as tr
from deeplearninginassetpricing_paperreplication_amd.data.dataset import MISSING_VALUE, AssetPricingDataset, load_splits
from deeplearninginassetpricing_paperreplication_amd.train import cli

THR = np.float32(MISSING_VALUE + 1)


def brute_force(x, rowok, fill_missing, fill_dead):
    T, N, F = x.shape
    y = np.empty((T, N, F), dtype=np.float32)
    cnt = np.zeros((T, F), dtype=np.int32)
    for t in range(T):
        for f in range(F):
            A = [i for i in range(N) if rowok[t, i] and x[t, i, f] > THR]
            m = len(A)
            cnt[t, f] = m
            for i in range(N):
                y[t, i, f] = fill_missing if rowok[t, i] else fill_dead
            for i in A:
                lt = sum(1 for j in A if x[t, j, f] < x[t, i, f])
                eq = sum(1 for j in A if x[t, j, f] == x[t, i, f])
                y[t, i, f] = np.float32(2 * lt + eq - m) / np.float32(2 * m)
    return y, cnt


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 7, 64])
def test_definition_matches_brute_force(N, F):
    x, rowok = rc.make_panel(3, N, F, seed=10 * N + F)
    y, cnt = tr.rank_characteristics_numpy(x, rowok, fill_missing=0.25, fill_dead=MISSING_VALUE)
    yb, cb = brute_force(x, rowok, np.float32(0.25), np.float32(MISSING_VALUE))
    assert np.array_equal(cnt, cb)
    assert np.array_equal(rc.bits(y), rc.bits(yb))
    if F == 5:                      # the empty column and the column with one participant (-> 0)
        assert cnt[0, 4] == 0 and cnt[0, 3] == 1 and y[0, 0, 3] == 0.0
    assert (cnt[2] == 0).all()      # the empty period
    part = rowok[:, :, None] & (x > THR)
    assert np.all(np.abs(y[part]) < 0.5)


def _clean(T=3, N=97, F=6, seed=3, scale=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, N, F)) * scale).astype(np.float32)
    x[:, :, 1] = rng.choice(rc.TIES, size=(T, N))
    x[:, :, 2] = np.round(x[:, :, 2] * 2) / 2          # ties among continuous values
    rowok = rng.random((T, N)) > 0.15
    return x, rowok


def test_antisymmetric():
    x, rowok = _clean(scale=20.0)
    x = np.clip(x, -89.0, 89.0)
    y, c = tr.rank_characteristics_numpy(x, rowok)
    yn, cn = tr.rank_characteristics_numpy(-x, rowok)
    assert np.array_equal(c, cn)
    live = np.broadcast_to(rowok[:, :, None], x.shape)
    assert np.array_equal(yn[live], -y[live])           # exact: k -> -k over the same 2 m


def test_scale_invariant():
    x, rowok = _clean()
    x = np.clip(x, -9.9, 9.9)
    y, c = tr.rank_characteristics_numpy(x, rowok)
    y8, c8 = tr.rank_characteristics_numpy(np.float32(8) * x, rowok)
    assert np.array_equal(c, c8) and np.array_equal(rc.bits(y), rc.bits(y8))


def test_numerators_sum_to_zero_and_distinct_keys_get_distinct_ranks():
    x, rowok = rc.make_panel(3, 200, 7, seed=5)
    y, cnt = tr.rank_characteristics_numpy(x, rowok)
    part = rowok[:, :, None] & (x > THR)
    for t in range(3):
        for f in range(7):
            p = part[t, :, f]
            m = int(cnt[t, f])
            assert m == p.sum()
            if not m:
                continue
            k = np.rint(y[t, p, f].astype(np.float64) * (2 * m)).astype(np.int64)
            assert k.sum() == 0
            assert np.all(np.abs(k) < m)
            v = x[t, p, f]
            assert len(np.unique(v)) == len(np.unique(y[t, p, f]))      # (-0 and +0 are one key)
            o = np.argsort(v, kind="stable")
            assert np.all(np.diff(y[t, p, f][o]) >= 0)
            if len(np.unique(v)) == m:                                  # no ties: the median is 0
                assert np.median(y[t, p, f]) == 0
    assert np.all(y[~rowok] == np.float32(MISSING_VALUE))
    assert np.all(y[rowok[:, :, None] & ~part] == 0.0)


def test_row_filter(shipped_data, tmp_path):
    with np.load(os.path.join(shipped_data, "char", "Char_valid.npz")) as z:
        data = z["data"].astype(np.float32)
    rng = np.random.default_rng(1)
    data[rng.random(data.shape) < 0.01] = np.float32(MISSING_VALUE)
    data[3, 5, 0] = np.nan
    ret, x = data[:, :, 0], data[:, :, 1:]
    F = x.shape[2]
    path = str(tmp_path / "Char_holes.npz")
    np.savez(path, data=data)
    ds = AssetPricingDataset(path)
    assert np.array_equal(tr.row_filter(ret, x, "none", 1), ds.mask)
    assert np.array_equal(tr.row_filter(ret, x, "none", F), ds.mask)       # (min_characteristics is not read)
    ret_ok = (ret > THR) & ~np.isnan(ret)
    present = (x > THR).sum(axis=2)
    for k in (1, F // 2, F):
        assert np.array_equal(tr.row_filter(ret, x, "median", k), ret_ok & (present >= k))
    assert np.array_equal(tr.row_filter(ret, x, "median", 0), ret_ok & (present >= 1))
    assert np.array_equal(tr.row_filter(ret, x, "median", F), ds.mask)
    with pytest.raises(ValueError):
        tr.row_filter(ret, x, "mean", 1)


@pytest.fixture(scope="module")
def raw_dir(shipped_data, tmp_path_factory):
    return rc.make_raw_dir(shipped_data, str(tmp_path_factory.mktemp("raw_panel")))


@pytest.mark.parametrize("impute,min_chars", [("none", 1), ("median", 40)])
def test_round_trip_through_the_loader(raw_dir, tmp_path, impute, min_chars, capsys):
    out = str(tmp_path / "prepared")
    rep_file = str(tmp_path / "report.json")
    report = tr.main(["--input_dir", raw_dir, "--output_dir", out, "--impute", impute, "--min_characteristics",
                      str(min_chars), "--device", "cpu", "--report", rep_file])
    assert "[prepare_data] train:" in capsys.readouterr().out
    assert json.load(open(rep_file)) == json.loads(json.dumps(report))
    splits = load_splits(out)
    for s, ds in zip(("train", "valid", "test"), splits):
        with np.load(os.path.join(raw_dir, "char", f"Char_{s}.npz")) as z:
            raw = {k: z[k] for k in z.files}
        ret, x = raw["data"][:, :, 0], raw["data"][:, :, 1:]
        rowok = tr.row_filter(ret, x, impute, min_chars)
        y, cnt = tr.rank_characteristics_numpy(x, rowok, 0.0, 0.0)
        assert np.array_equal(ds.mask, rowok)
        assert np.array_equal(rc.bits(ds.individual_features), rc.bits(y))
        assert np.array_equal(rc.bits(ds.returns), rc.bits(np.where(rowok, ret, np.float32(0))))
        with np.load(os.path.join(out, "char", f"Char_{s}.npz")) as z:
            assert sorted(z.files) == sorted(raw)
            for k in raw:
                if k != "data":
                    assert np.array_equal(z[k], raw[k])
            assert np.all(z["data"][~rowok] == np.float32(MISSING_VALUE))
        assert filecmp.cmp(os.path.join(raw_dir, "macro", f"macro_{s}.npz"),
                           os.path.join(out, "macro", f"macro_{s}.npz"), shallow=False)
        r = report[s]
        ret_ok = (ret > THR) & ~np.isnan(ret)
        complete = ret_ok & ((x > THR).sum(axis=2) == x.shape[2])
        assert (r["T"], r["N"], r["F"]) == x.shape
        assert r["rows_with_return"] == ret_ok.sum() and r["complete_rows"] == complete.sum()
        assert r["kept_rows"] == rowok.sum()
        assert np.allclose(r["coverage"], cnt.sum(axis=0) / rowok.sum(), rtol=0, atol=1e-12)
        if impute == "none":        # complete rows only: every column is fully covered
            assert r["kept_rows"] == complete.sum() < ret_ok.sum()
            assert min(r["coverage"]) == 1.0
        else:                       # rows with single gaps are kept and the gaps show in the coverage
            assert complete.sum() < r["kept_rows"] <= ret_ok.sum()
            assert 0.9 < min(r["coverage"]) and max(r["coverage"]) < 1.0
        assert r["impute"] == impute and r["min_characteristics"] == min_chars and r["device"] == "cpu"


def test_preparing_a_prepared_panel_changes_nothing(raw_dir):
    with np.load(os.path.join(raw_dir, "char", "Char_valid.npz")) as z:
        data = z["data"]
    once, r1 = tr.prepare_split(data, "none", 1, "cpu")
    twice, r2 = tr.prepare_split(once, "none", 1, "cpu")
    assert once.tobytes() == twice.tobytes()
    assert r1["kept_rows"] == r2["kept_rows"] == r2["rows_with_return"] > 0


def test_training_runs_on_a_prepared_directory(raw_dir, tmp_path):
    out = str(tmp_path / "prepared")
    tr.prepare_data_dir(raw_dir, out, impute="median", min_characteristics=23, device="cpu")
    _, history = cli.main(["--data_dir", out, "--small_sample", "--n_periods", "12", "--n_stocks", "40",
                           "--epochs_unc", "2", "--epochs_moment", "1", "--epochs", "2", "--ignore_epoch", "0",
                           "--print_freq", "1", "--save_dir", str(tmp_path / "run"), "--device", "cpu"])
    losses = [np.asarray(v, dtype=np.float64) for k, v in history.items() if "loss" in k]
    assert losses and all(v.size and np.isfinite(v).all() for v in losses)

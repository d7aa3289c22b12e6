"""Double-sorted portfolios (``analysis.sorted_portfolios``) on the CPU: ``double_sort_numpy``
against a brute-force per-row implementation of the definition (ties, an empty period, a period
with n < Qa, both modes), its independent-mode marginals against the single sort, the tie-free
conditional cell sizes, the argument checks, the pricing of a tiny panel against a direct float64
evaluation, and the evaluator's flags."""
import json
import math
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

PAIRS = [(0, 1), (1, 0), (2, 3), (3, 3), (1, 2)]


def _panel():
    """6 x 40 x 4: column 1 has 3 distinct values, column 2 signed zeros and ties; period 3 is
    empty, period 4 has 2 stocks and period 5 one (n < Qa)."""
    rng = np.random.default_rng(3)
    keys = rng.standard_normal((6, 40, 4)).astype(np.float32)
    keys[:, :, 1] = rng.integers(0, 3, (6, 40)).astype(np.float32)
    keys[:, ::4, 2] = -0.0
    keys[:, 1::4, 2] = 0.0
    keys[:, 2::8, 2] = 0.5
    mask = rng.random((6, 40)) > 0.2
    mask[3] = False
    mask[4] = False
    mask[4, [7, 21]] = True
    mask[5] = False
    mask[5, 12] = True
    vals = rng.standard_normal((6, 40, 2))
    return keys, mask, vals


def _bp(sorted_list, Q):
    n = len(sorted_list)
    return [sorted_list[math.ceil(d * n / Q) - 1] for d in range(1, Q)]


def _brute(keys, pairs, mask, vals, Qa, Qb, conditional):
    """The definition, row by row, on python floats and sorted() lists."""
    T, N, _ = keys.shape
    V = vals.shape[2]
    P = len(pairs)
    count = np.zeros((T, P, Qa, Qb), np.int64)
    sums = np.zeros((T, P, Qa, Qb, V))
    ba = np.full((T, P, Qa - 1), np.nan)
    bb = np.full((T, P, Qa, Qb - 1), np.nan)
    for t in range(T):
        rows = [i for i in range(N) if mask[t, i]]
        if not rows:
            continue
        for p, (ca, cb) in enumerate(pairs):
            A = {i: float(keys[t, i, ca]) + 0.0 for i in rows}
            B = {i: float(keys[t, i, cb]) + 0.0 for i in rows}
            bA = _bp(sorted(A.values()), Qa)
            ba[t, p] = bA
            qa = {i: sum(1 for b in bA if A[i] > b) for i in rows}
            if conditional:
                bB = {}
                for a in range(Qa):
                    members = [i for i in rows if qa[i] == a]
                    if members:
                        bB[a] = _bp(sorted(B[i] for i in members), Qb)
                        bb[t, p, a] = bB[a]
            else:
                one = _bp(sorted(B.values()), Qb)
                bB = {a: one for a in range(Qa)}
                bb[t, p, :] = one
            for i in rows:
                qb = sum(1 for b in bB[qa[i]] if B[i] > b)
                count[t, p, qa[i], qb] += 1
                sums[t, p, qa[i], qb] += vals[t, i]
    return count, sums, ba, bb


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("Q", [(5, 5), (2, 3), (3, 12), (6, 6)])
def test_numpy_matches_brute_force(Q, conditional):
    keys, mask, vals = _panel()
    got = sp.double_sort_numpy(keys, PAIRS, mask, vals, Q, conditional)
    count, sums, ba, bb = _brute(keys, PAIRS, mask, vals, Q[0], Q[1], conditional)
    assert got["count"].dtype == np.int32 and got["sum"].dtype == np.float64
    assert got["breaks_a"].dtype == np.float32 and got["breaks_b"].dtype == np.float32
    assert got["count"].shape == (6, len(PAIRS), Q[0], Q[1]) and got["sum"].shape == (6, len(PAIRS), Q[0], Q[1], 2)
    np.testing.assert_array_equal(got["count"], count)
    np.testing.assert_array_equal(got["breaks_a"], ba.astype(np.float32))
    np.testing.assert_array_equal(got["breaks_b"], bb.astype(np.float32))
    assert not np.signbit(got["breaks_b"][got["breaks_b"] == 0]).any()       # -0.0 is folded onto +0.0
    np.testing.assert_allclose(got["sum"], sums, rtol=0, atol=1e-12)
    assert (got["count"].sum((-1, -2)) == mask.sum(1)[:, None]).all()
    assert got["rows"] == mask.sum()
    # the empty period, and n = 2 < Qa
    assert got["count"][3].sum() == 0 and np.isnan(got["breaks_a"][3]).all() and np.isnan(got["breaks_b"][3]).all()
    assert (got["sum"][3] == 0).all()
    assert ((got["count"][4] > 0).sum((-1, -2)) <= 2).all() and ((got["count"][5] > 0).sum((-1, -2)) == 1).all()
    if conditional:         # a first-key bucket without rows: NaN breakpoints; with rows: finite ones
        na = got["count"].sum(-1)
        assert (np.isnan(got["breaks_b"]).all(-1) == (na == 0)).all()
        assert (np.isfinite(got["breaks_b"]).all(-1) == (na > 0)).all()
    else:                   # one set of B breakpoints per period
        for a in range(1, Q[0]):
            np.testing.assert_array_equal(got["breaks_b"][:, :, a], got["breaks_b"][:, :, 0])


def test_membership_does_not_depend_on_the_stock_order():
    keys, mask, vals = _panel()
    perm = np.random.default_rng(0).permutation(40)
    a = sp.double_sort_numpy(keys, PAIRS, mask, vals, (4, 4))
    b = sp.double_sort_numpy(keys[:, perm], PAIRS, mask[:, perm], vals[:, perm], (4, 4))
    np.testing.assert_array_equal(a["count"], b["count"])
    np.testing.assert_array_equal(a["breaks_b"], b["breaks_b"])
    np.testing.assert_allclose(a["sum"], b["sum"], rtol=0, atol=1e-12)


def test_independent_mode_marginals_equal_the_single_sort():
    keys, mask, vals = _panel()
    Qa, Qb = 4, 7
    got = sp.double_sort_numpy(keys, PAIRS, mask, vals, (Qa, Qb), conditional=False)
    sa = sp.sort_buckets_numpy(keys, mask, vals, Qa)
    sb = sp.sort_buckets_numpy(keys, mask, vals, Qb)
    for p, (ca, cb) in enumerate(PAIRS):
        np.testing.assert_array_equal(got["count"][:, p].sum(-1), sa["count"][:, ca])
        np.testing.assert_array_equal(got["breaks_a"][:, p], sa["breaks"][:, ca])
        np.testing.assert_array_equal(got["count"][:, p].sum(-2), sb["count"][:, cb])
        np.testing.assert_array_equal(got["breaks_b"][:, p, 0], sb["breaks"][:, cb])
        np.testing.assert_allclose(got["sum"][:, p].sum(-2), sa["sum"][:, ca], rtol=0, atol=1e-12)
    # the conditional sort keeps the first key's marginal
    cond = sp.double_sort_numpy(keys, PAIRS, mask, vals, (Qa, Qb), conditional=True)
    np.testing.assert_array_equal(cond["count"].sum(-1), got["count"].sum(-1))
    np.testing.assert_array_equal(cond["breaks_a"], got["breaks_a"])


@pytest.mark.parametrize("Q", [(5, 5), (3, 12), (16, 2)])
def test_tie_free_conditional_cells_are_balanced(Q):
    rng = np.random.default_rng(8)
    keys = rng.standard_normal((4, 83, 3))
    mask = rng.random((4, 83)) > 0.1
    got = sp.double_sort_numpy(keys, [(0, 1), (2, 0), (1, 1)], mask, np.ones((4, 83, 1)), Q)
    assert got["breaks_a"].dtype == np.float64
    cnt = got["count"]
    na = cnt.sum(-1, keepdims=True)
    n = mask.sum(1)[:, None, None]
    assert (cnt.sum(-1) >= n // Q[0]).all() and (cnt.sum(-1) <= -(-n // Q[0])).all()
    ok = na > 0
    assert (np.where(ok, cnt >= na // Q[1], True)).all() and (np.where(ok, cnt <= -(-na // Q[1]), True)).all()


def test_argument_checks():
    keys, mask, vals = _panel()
    for q in [(6, 7), (4, 10), (1, 5), (5, 1), (17, 2), (2, 17), 5, (5, 5, 5)]:
        with pytest.raises(ValueError):
            sp.double_sort_numpy(keys, PAIRS, mask, vals, q)
    with pytest.raises(ValueError):
        sp.double_sort_numpy(keys, [(0, 4)], mask, vals)
    with pytest.raises(ValueError):
        sp.double_sort_numpy(keys, [(-1, 0)], mask, vals)
    assert sp.double_sort_numpy(keys, [], mask, vals)["count"].shape == (6, 0, 5, 5)
    assert sp.double_sort_numpy(keys, [(0, 0)], mask, vals, (6, 6))["count"].shape == (6, 1, 6, 6)
    assert sp.parse_double_quantiles("5x5") == (5, 5) and sp.parse_double_quantiles("3X12") == (3, 12)
    assert sp.parse_double_quantiles((2, 4)) == (2, 4)
    for bad in ("5", "5x", "axb", "7x6", "1x5", "5x5x5"):
        with pytest.raises(ValueError):
            sp.parse_double_quantiles(bad)


def test_price_double_sorted_against_a_direct_evaluation():
    rng = np.random.default_rng(4)
    T, N, P, Qa, Qb = 7, 12, 2, 2, 3
    w = rng.standard_normal((T, N))
    r = 0.1 * rng.standard_normal((T, N))
    mask = rng.random((T, N)) > 0.15
    cnt = rng.integers(0, 3, (T, P, Qa, Qb)).astype(np.int32)
    cnt[:, 1, 1, 2] = 0                                   # an asset that never exists
    cnt[1:, 1, 0, 0] = 0                                  # an asset with a single period
    ret = np.where(cnt > 0, 0.1 * rng.standard_normal(cnt.shape), np.nan)
    load = np.where(cnt > 0, rng.standard_normal(cnt.shape), np.nan)
    res = {"returns": ret, "loading": load, "count": cnt, "names": ["a x b", "c x weight"], "pairs": [(0, 1), (2, 3)],
           "quantiles": (Qa, Qb), "mode": "conditional"}
    got = sp.price_double_sorted(res, w, r, mask)
    beta = np.array([(r[t] * w[t] * mask[t]).sum() / (w[t] * w[t] * mask[t]).sum() for t in range(T)])
    me2 = np.full((P, Qa, Qb), np.nan)
    mr2 = np.full((P, Qa, Qb), np.nan)
    for p in range(P):
        for a in range(Qa):
            for b in range(Qb):
                ts = [t for t in range(T) if cnt[t, p, a, b] > 0]
                if not ts:
                    assert np.isnan(got["mean_ret"][p, a, b]) and np.isnan(got["alpha"][p, a, b])
                    continue
                rr = np.array([ret[t, p, a, b] for t in ts])
                ee = np.array([ret[t, p, a, b] - beta[t] * load[t, p, a, b] for t in ts])
                assert got["mean_ret"][p, a, b] == pytest.approx(rr.mean(), rel=1e-12)
                assert got["alpha"][p, a, b] == pytest.approx(ee.mean(), rel=1e-10)
                assert got["ev_asset"][p, a, b] == pytest.approx(1 - (ee ** 2).sum() / (rr ** 2).sum(), rel=1e-10)
                if len(ts) > 1:
                    assert got["t_alpha"][p, a, b] == pytest.approx(ee.mean() / (ee.std(ddof=1) / np.sqrt(len(ts))), rel=1e-9)
                else:
                    assert np.isnan(got["t_alpha"][p, a, b])
                me2[p, a, b], mr2[p, a, b] = (ee ** 2).mean(), (rr ** 2).mean()
        has = np.isfinite(me2[p])
        assert got["pair_ev"][p] == pytest.approx(1 - me2[p][has].sum() / mr2[p][has].sum(), rel=1e-10)
        al, mr = got["alpha"][p][has], got["mean_ret"][p][has]
        assert got["pair_xs_r2"][p] == pytest.approx(1 - (al ** 2).mean() / (mr ** 2).mean(), rel=1e-10)
        assert got["pair_mean_abs_alpha"][p] == pytest.approx(np.abs(al).mean(), rel=1e-10)
        both = [t for t in range(T) if cnt[t, p, 0, 0] > 0 and cnt[t, p, Qa - 1, Qb - 1] > 0]
        if both:
            sprd = np.array([ret[t, p, Qa - 1, Qb - 1] - ret[t, p, 0, 0] for t in both])
            assert got["hml"][p] == pytest.approx(sprd.mean(), rel=1e-10)
            if sprd.std() > 0:
                assert got["hml_sharpe"][p] == pytest.approx(sprd.mean() / sprd.std(), rel=1e-9)
        else:
            assert np.isnan(got["hml"][p])
    assert np.isnan(got["hml"][1])                        # cell (1, 2) of pair 1 never exists
    has = np.isfinite(me2)
    assert got["assets"] == has.sum() == P * Qa * Qb - 1
    assert got["ev"] == pytest.approx(1 - me2[has].sum() / mr2[has].sum(), rel=1e-10)
    assert got["xs_r2"] == pytest.approx(1 - (got["alpha"][has] ** 2).mean() / (got["mean_ret"][has] ** 2).mean(), rel=1e-10)
    assert got["mean_abs_alpha"] == pytest.approx(np.abs(got["alpha"][has]).mean(), rel=1e-10)
    lines = sp.format_double_sorted(got)
    assert len(lines) == 1 + P * (1 + Qa) and "EV" in lines[0] and "corner H-L" in lines[1]
    d = json.loads(json.dumps(sp.double_to_json(res, got), allow_nan=False))
    assert d["mean_ret"][1][1][2] is None and d["quantiles"] == [2, 3] and d["mode"] == "conditional"


@pytest.fixture(scope="module")
def setup():
    T, N, F, M = 5, 40, 6, 3
    g = torch.Generator().manual_seed(5)
    batch = {
        "individual_features": torch.randn(T, N, F, generator=g),
        "macro_features": torch.randn(T, M, generator=g),
        "returns": 0.1 * torch.randn(T, N, generator=g),
        "mask": torch.rand(T, N, generator=g) > 0.25,
    }
    cfg = default_cli_config(M, F, hidden_dim=[8], rnn_dim=[2], dropout=0.05)
    models = []
    for s in (0, 1):
        torch.manual_seed(30 + s)
        models.append(AssetPricingGAN(cfg).eval())
    return models, batch


def test_double_sorted_portfolios_cpu(setup):
    models, batch = setup
    T, N, F = batch["individual_features"].shape
    res = sp.double_sorted_portfolios(models, batch, [(0, 1), ("weight", "c"), (2, F)], quantiles=(3, 2),
                                      names=list("abcdef"))
    assert res["pairs"] == [(0, 1), (F, 2), (2, F)] and res["names"] == ["a x b", "weight x c", "c x weight"]
    assert res["quantiles"] == (3, 2) and res["mode"] == "conditional" and "gpu_ms" not in res
    assert res["returns"].shape == res["loading"].shape == res["count"].shape == (T, 3, 3, 2)
    assert res["breaks_a"].shape == (T, 3, 2) and res["breaks_b"].shape == (T, 3, 3, 1)
    mask = batch["mask"].numpy()
    assert (res["count"].sum((-1, -2)) == mask.sum(1)[:, None]).all()
    w = sp._cpu_weights(models, batch)
    # sorted on the weight first, then on the weight within: the loadings rise along both axes
    ww = sp.double_sorted_portfolios(models, batch, [("weight", "weight")], quantiles=(3, 2), weights=w)
    flat = ww["loading"][:, 0].reshape(T, 6)
    assert (np.diff(flat, axis=1) > 0).all()
    # cell means by hand for one period and pair
    t, (ca, cb) = 1, (0, 1)
    k = batch["individual_features"].numpy()
    idx = np.nonzero(mask[t])[0]
    qa = np.argsort(np.argsort(k[t, idx, ca])) * 3 // len(idx)
    r = batch["returns"].numpy()
    for a in range(3):
        ia = idx[qa == a]
        qb = np.argsort(np.argsort(k[t, ia, cb])) * 2 // len(ia)
        for b in range(2):
            assert res["count"][t, 0, a, b] == (qb == b).sum()
            assert res["returns"][t, 0, a, b] == pytest.approx(r[t, ia[qb == b]].astype(np.float64).mean(), abs=1e-12)
            assert res["loading"][t, 0, a, b] == pytest.approx(w[t, ia[qb == b]].astype(np.float32).astype(np.float64).mean(), abs=1e-12)
    ind = sp.double_sorted_portfolios(models, batch, [(0, 1)], quantiles=(3, 2), conditional=False, weights=w)
    assert ind["mode"] == "independent" and (ind["breaks_b"][:, 0, 0] == ind["breaks_b"][:, 0, 2]).all()
    for bad in ([(0, 7)], [(-1, 0)], [("nope", 0)], [(0, 1, 2)]):
        with pytest.raises(ValueError):
            sp.double_sorted_portfolios(models, batch, bad)
    with pytest.raises(ValueError):
        sp.double_sorted_portfolios(models, batch, [(0, 1)], quantiles=(7, 6))
    with pytest.raises(ValueError):
        sp.double_sorted_portfolios([], batch, [(0, 1)])
    priced = sp.price_double_sorted(res, w, r, mask)
    assert priced["mean_ret"].shape == (3, 3, 2) and priced["pair_ev"].shape == (3,)
    json.dumps(sp.double_to_json(res, priced), allow_nan=False)


def test_cli_flag_parsing(monkeypatch):
    a = ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1", "c2"])
    assert a.double_sorts is None and a.double_quantiles == "5x5" and a.double_mode == "conditional" and a.double_out is None
    assert "double_sorts" not in ens._extra_kwargs(a)
    a = ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1", "--double_sorts", "size:bm,weight:3",
                                  "--double_quantiles", "3x4", "--double_mode", "independent", "--double_out", "o.json",
                                  "--sort_split", "valid"])
    kw = ens._extra_kwargs(a)
    assert kw == {"double_sorts": "size:bm,weight:3", "double_quantiles": (3, 4), "double_mode": "independent",
                  "double_out": "o.json", "sort_split": "valid"}
    with pytest.raises(SystemExit):
        ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1", "--double_mode", "both"])
    a = ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1", "--double_sorts", "0:1", "--double_quantiles", "7x6"])
    with pytest.raises(ValueError):
        ens._extra_kwargs(a)
    seen = {}
    monkeypatch.setattr(ens, "evaluate_ensemble", lambda *args, **kw: seen.update(kw) or "ret")
    assert ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--double_sorts", "0:1"]) == "ret"
    assert seen["double_sorts"] == "0:1" and seen["double_quantiles"] == (5, 5) and seen["double_mode"] == "conditional"


def _ckpts():
    return [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]


def test_cli_end_to_end_on_the_shipped_checkpoints(shipped_data, tmp_path, capsys):
    base = ens.evaluate_ensemble(_ckpts(), shipped_data, verbose=False)
    capsys.readouterr()
    out = tmp_path / "double.json"
    got = ens.main(["--data_dir", shipped_data, "--checkpoint_dirs", *_ckpts(), "--double_sorts", "0:1,weight:3",
                    "--double_quantiles", "3x4", "--sort_split", "valid", "--double_out", str(out)])
    text = capsys.readouterr().out
    assert "DOUBLE-SORTED PORTFOLIOS (valid split, 3 x 4 cells, conditional" in text
    assert set(got) == set(base) | {"double_sorts"}
    for k in base:
        assert got[k] == base[k]
    ds = got["double_sorts"]
    assert ds["portfolios"]["pairs"] == [(0, 1), (46, 3)] and ds["portfolios"]["count"].shape[1:] == (2, 3, 4)
    assert ds["portfolios"]["names"][1].startswith("weight x ")
    assert ds["priced"]["assets"] == 24 and np.isfinite(ds["priced"]["pair_ev"]).all()
    d = json.loads(out.read_text())
    assert {"names", "pairs", "quantiles", "mode", "periods", "count", "mean_ret", "alpha", "t_alpha", "ev_asset",
            "pair_ev", "pair_xs_r2", "pair_mean_abs_alpha", "hml", "hml_sharpe", "ev", "xs_r2", "mean_abs_alpha",
            "assets"} <= set(d)
    assert np.asarray(d["mean_ret"], dtype=float).shape == (2, 3, 4) and d["quantiles"] == [3, 4]
    ind = ens.evaluate_ensemble(_ckpts(), shipped_data, verbose=False, double_sorts=[(0, "weight")],
                                double_quantiles=(2, 2), double_mode="independent")
    assert ind["double_sorts"]["portfolios"]["mode"] == "independent"
    with pytest.raises(ValueError):
        ens.evaluate_ensemble(_ckpts(), shipped_data, verbose=False, double_sorts="0:1", double_mode="both")

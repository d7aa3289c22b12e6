"""Stock-level weights of a combination of tree nodes on the CPU (``tree_sorts.tree_weights_numpy``, the
definition) and of the pruned SDF (``tree_prune.node_coefficients`` / ``pruned_weights``): the vectorised
definition against the plain per-row loop bit for bit, the recount of the nodes, the identity
``sum_i w R = sum_nodes coef x mean return``, the skipping rules, the argument checks and the evaluator's
``--prune_metrics`` flag."""
import json
import os
import re

import numpy as np
import pytest

import golden_cases as gc
import weight_cases as wc
from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
from deeplearninginassetpricing_paperreplication_amd.analysis.portfolio import sharpe_ddof0


def _numpy(splits, coef, dtype=np.float32, trees=None, raw=None):
    keys, mask, _ = wc.small_panel()
    tr, rw = wc.small_sort(splits)
    trees, raw = (tr if trees is None else trees), (rw if raw is None else raw)
    return ts.tree_weights_numpy(keys, trees, mask, splits, raw["breaks"], raw["count"], coef, dtype=dtype)


@pytest.mark.parametrize("splits", wc.SMALL_SPLITS)
def test_numpy_is_the_row_loop(splits):
    keys, mask, _ = wc.small_panel()
    trees, raw = wc.small_sort(splits)
    P, NN = len(trees), raw["count"].shape[2]
    assert (1,) * len(splits) in trees                                   # a repeated key
    assert (raw["count"][3] == 0).all() and (raw["count"][1, :, 0] == 5).all()
    for coef in (wc.dense_coef(P, NN, 1, decades=3), wc.sparse_coef(P, splits)):
        want = wc.loop_weights(keys, trees, mask, splits, raw["breaks"], raw["count"], coef)
        a64 = _numpy(splits, coef, np.float64)
        w32 = _numpy(splits, coef)
        assert a64.dtype == np.float64 and w32.dtype == np.float32 and a64.shape == mask.shape
        np.testing.assert_array_equal(wc.bits64(a64), wc.bits64(want))
        np.testing.assert_array_equal(wc.bits32(w32), wc.bits32(want.astype(np.float32)))
        assert (wc.bits64(a64)[~mask] == 0).all()                        # invalid cells: +0.0
    assert (wc.bits64(a64)[mask] != 0).any()


@pytest.mark.parametrize("splits", [(2, 2, 2), (3, 4)])
def test_recounting_the_visited_nodes_gives_the_sort_s_counts(splits):
    """A one-hot coefficient marks the rows of one node: their number is ``count`` of the sort, and each
    carries ``1 / count``."""
    _, mask, _ = wc.small_panel()
    trees, raw = wc.small_sort(splits)
    P, NN = len(trees), raw["count"].shape[2]
    for p in (0, 2, 5):
        for j in range(NN):
            coef = np.zeros((P, NN))
            coef[p, j] = 1.0
            a = _numpy(splits, coef, np.float64)
            np.testing.assert_array_equal((a != 0).sum(axis=1), raw["count"][:, p, j])
            for t in range(mask.shape[0]):
                if raw["count"][t, p, j]:
                    assert set(a[t][a[t] != 0]) == {1.0 / raw["count"][t, p, j]}


@pytest.mark.parametrize("splits", wc.SMALL_SPLITS)
def test_weighted_returns_are_the_node_returns(splits):
    """``sum_i acc R = sum_nodes coef x mean return`` per period: both sides are the products ``coef R / count`` in
    another order, so they agree within ``n 2^-52 sum_i |acc R|`` plus one ulp (the node-sum bound)."""
    keys, mask, ret = wc.small_panel()
    trees, raw = wc.small_sort(splits)
    P, NN = len(trees), raw["count"].shape[2]
    coef = wc.dense_coef(P, NN, 2)
    a = _numpy(splits, coef, np.float64)
    r = ret.astype(np.float64) * mask
    lhs = (a * r).sum(axis=1)
    cnt = raw["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, raw["sum"][..., 0] / cnt, 0.0)
    rhs = (coef[None] * mean).sum(axis=(1, 2))
    bound = wc.node_sum_bound(mask.sum(axis=1), np.abs(a * r).sum(axis=1), rhs)
    dev = np.abs(lhs - rhs)
    print(f"largest |sum_i acc R - sum coef mean| / bound = {float((dev / bound).max()):.3f}")
    assert (dev <= bound).all() and np.abs(rhs).max() > 0


def _sharpe_bound(f, e):
    """First-order bound on the change of mean / std when every ``f[t]`` moves by at most ``e[t]``, doubled
    for the higher orders: ``d SR / d f_t = (1 - SR (f_t - mean) / sd) / (T sd)``."""
    T, m, sd = f.shape[0], f.mean(), f.std()
    g = np.abs(1.0 - (m / sd) * (f - m) / sd) / (T * sd)
    return 2.0 * float((g * e).sum())


def test_pruned_weights_reproduce_the_factor():
    pr, by_split, batches = wc.planted_case()
    pw = tp.pruned_weights(pr, by_split, batches, [], device="cpu")
    assert set(pw) == set(tp.SPLITS)
    worst = 0.0
    for s in tp.SPLITS:
        b = {k: v.numpy() for k, v in batches[s].items()}
        w = pw[s]
        assert w.dtype == np.float32 and w.shape == b["mask"].shape and (wc.bits32(w)[~b["mask"]] == 0).all()
        ref = tp.node_returns(by_split[s], pr["depth_weight"])[0] @ pr["theta"]
        f = tp.factor_from_weights(w, b["returns"], b["mask"])
        absum = (np.abs(w.astype(np.float64) * b["returns"].astype(np.float64)) * b["mask"]).sum(axis=1)
        # the float32 rounding of w (2^-24 relative per stock) plus the two orders of the same float64 products
        bound = 2.0 ** -24 * absum + wc.node_sum_bound(b["mask"].sum(axis=1), absum, ref)
        dev = np.abs(f - ref)
        print(f"{s}: largest |sum_i w R - R . theta| = {dev.max():.3e}, / bound = {float((dev / bound).max()):.3f}")
        assert (dev <= bound).all() and np.abs(ref).max() > 0
        worst = max(worst, float(dev.max()))
        assert abs(sharpe_ddof0(f) - pr[s + "_sharpe"]) <= _sharpe_bound(ref, bound)
    pm = tp.pruned_metrics(pr, by_split, pw, batches)
    assert set(pm) == {"train_sharpe", "valid_sharpe", "test_sharpe", "ev", "xs_r2", "turnover", "max_1m_loss_std", "self_check"}
    assert pm["self_check"] == worst and all(np.isfinite(v) for v in pm.values())
    lines = tp.format_pruned_metrics(pm, gan={"ev": 0.1, "xs_r2": 0.2, "turnover": 0.3, "max_1m_loss_std": 4.0})
    assert any("Pruned trees" in x for x in lines) and any("Ensemble" in x for x in lines) and "Self-check" in lines[-1]


@pytest.mark.parametrize("splits", [(2, 2, 2), (3, 4)])
def test_zero_trees_and_zero_levels_change_no_bit(splits):
    keys, mask, _ = wc.small_panel()
    trees, raw = wc.small_sort(splits)
    P, NN = len(trees), raw["count"].shape[2]
    lay = ts.tree_layout(splits)
    off, boff = lay["level_offsets"], lay["break_offsets"]
    coef = wc.dense_coef(P, NN, 3, decades=2)
    coef[[0, 3, P - 1]] = 0.0                                            # three all-zero trees
    coef[2, off[2]:] = 0.0                                               # tree 2 stops at level 1
    full = _numpy(splits, coef, np.float64)
    # the call without its all-zero trees
    keep = [p for p in range(P) if np.any(coef[p] != 0)]
    assert len(keep) == P - 3
    sub = {k: np.ascontiguousarray(raw[k][:, keep]) for k in ("breaks", "count")}
    got = _numpy(splits, coef[keep], np.float64, trees=[trees[p] for p in keep], raw=sub)
    np.testing.assert_array_equal(wc.bits64(got), wc.bits64(full))
    # every tree stopped at level 1: the one-level call on the prefix of the tables (the layout is level order)
    c1 = coef.copy()
    c1[:, off[2]:] = 0.0
    deep = _numpy(splits, c1, np.float64)
    short = ts.tree_weights_numpy(keys, [tr[:1] for tr in trees], mask, splits[:1], raw["breaks"][:, :, :boff[1]],
                                  raw["count"][:, :, :off[2]], c1[:, :off[2]], dtype=np.float64)
    np.testing.assert_array_equal(wc.bits64(deep), wc.bits64(short))
    # levels below the deepest non-zero one are not read: NaN breakpoints and zero counts there change nothing
    junk = {"breaks": raw["breaks"].copy(), "count": raw["count"].copy()}
    junk["breaks"][:, :, boff[1]:] = np.nan
    junk["count"][:, :, off[2]:] = 0
    np.testing.assert_array_equal(wc.bits64(_numpy(splits, c1, np.float64, raw=junk)), wc.bits64(deep))


def test_negative_zero_coefficients_are_zero():
    splits = (2, 2, 2)
    trees, raw = wc.small_sort(splits)
    coef = wc.sparse_coef(len(trees), splits)
    neg = np.where(coef == 0, -0.0, coef)
    assert np.signbit(neg).sum() > np.signbit(coef).sum()
    np.testing.assert_array_equal(wc.bits64(_numpy(splits, neg, np.float64)), wc.bits64(_numpy(splits, coef, np.float64)))
    # an all -0.0 table: every weight is +0.0
    assert (wc.bits64(_numpy(splits, np.full_like(coef, -0.0), np.float64)) == 0).all()


def test_argument_checks_and_foreign_breakpoints():
    splits = (2, 2, 2)
    keys, mask, _ = wc.small_panel()
    trees, raw = wc.small_sort(splits)
    P, NN = len(trees), raw["count"].shape[2]
    coef = wc.dense_coef(P, NN, 4)
    # another panel's keys: rows walk into nodes that the counts call empty (period 1 has 5 rows, 8 leaves)
    with pytest.raises(ValueError, match="empty node"):
        ts.tree_weights_numpy(keys + np.float32(100.0), trees, mask, splits, raw["breaks"], raw["count"], coef)
    for bad in (coef[:-1], coef[:, :-1], np.where(np.arange(NN) == 3, np.nan, coef), np.where(np.arange(NN) == 3, np.inf, coef)):
        with pytest.raises(ValueError):
            _numpy(splits, bad)
    with pytest.raises(ValueError, match="breaks must be"):
        ts.tree_weights_numpy(keys, trees, mask, splits, raw["breaks"][:, :, :-1], raw["count"], coef)
    with pytest.raises(ValueError, match="breaks must be"):
        ts.tree_weights_numpy(keys, trees, mask, splits, raw["breaks"], raw["count"][:, :-1], coef)
    with pytest.raises(ValueError, match="dtype"):
        _numpy(splits, coef, np.float16)
    assert ts.active_keys(trees, splits, np.zeros((P, NN))) == []
    # tree 1 is active down to level 1, tree P - 2 down to its leaves
    assert ts.active_keys(trees, splits, wc.sparse_coef(P, splits)) == list(dict.fromkeys([trees[1][0], *trees[P - 2]]))


def test_node_coefficients_sit_at_the_representatives():
    pr, by_split, _ = wc.planted_case()
    res = by_split["train"]
    un = ts.unique_nodes(res["trees"], res["splits"])
    lay = ts.tree_layout(res["splits"])
    theta = np.arange(1.0, len(un["nodes"]) + 1.0)                       # every distinct node non-zero
    for dw in (True, False):
        coef = tp.node_coefficients({"theta": theta, "depth_weight": dw}, res)
        assert coef.shape == (len(res["trees"]), lay["nodes"]) and coef.dtype == np.float64
        assert int((coef != 0).sum()) == len(un["nodes"]) < coef.size   # shared nodes (the root, equal paths) once
        for u, ((p, j), lev) in enumerate(zip(un["nodes"], un["levels"])):
            fac = 1.0 / np.sqrt(float(lay["nodes_per_level"][lev])) if dw else 1.0
            assert coef[p, j] == theta[u] * fac
        assert coef[0, 0] == theta[0] and (coef[1:, 0] == 0).all()       # the root: tree 0 only
    sel = tp.node_coefficients(pr, res)
    assert int((sel != 0).sum()) == len(pr["nodes"])
    for tr, nd, _, lev, wgt in pr["nodes"]:
        assert sel[tr, nd] == wgt * (1.0 / np.sqrt(float(lay["nodes_per_level"][lev])))
    with pytest.raises(ValueError, match="distinct nodes"):
        tp.node_coefficients({"theta": theta[:-1]}, res)


def test_tree_weights_on_the_cpu_needs_no_model_without_the_weight_key():
    pr, by_split, batches = wc.planted_case()
    res, b = by_split["valid"], batches["valid"]
    coef = tp.node_coefficients(pr, res)
    out = ts.tree_weights([], b, res, coef, acc=True)
    want = ts.tree_weights_numpy(b["individual_features"].numpy(), res["trees"], b["mask"].numpy(), res["splits"], res["breaks"],
                                 res["count"], coef, dtype=np.float64)
    np.testing.assert_array_equal(wc.bits64(out["acc"]), wc.bits64(want))
    np.testing.assert_array_equal(wc.bits32(out["w"]), wc.bits32(want.astype(np.float32)))
    assert "gpu_ms" not in out


def test_python_layer_with_trees_that_sort_on_the_weight():
    """``weight`` (key F) in a level that is read, below a tree's deepest non-zero level, in a tree without a
    coefficient and in a tree of which only the root is selected."""
    import torch
    keys, mask, ret = wc.small_panel()
    rng = np.random.default_rng(9)
    wgt = rng.standard_normal(mask.shape).astype(np.float32)
    b = {"returns": torch.from_numpy(ret), "individual_features": torch.from_numpy(keys), "mask": torch.from_numpy(mask)}
    trees, splits = [("weight", 1, 2), (1, 2, "weight"), (5, 5, 5), (3, "weight", 4), (0, 1, 2)], (2, 2, 2)
    res = ts.tree_sorted_portfolios([], b, trees, splits=splits, weights=wgt)
    assert res["trees"][0] == (5, 1, 2)
    off = ts.tree_layout(splits)["level_offsets"]
    coef = wc.dense_coef(5, 15, 32)
    coef[1, off[3]:] = 0.0
    coef[2] = 0.0
    coef[3, 1:] = 0.0
    full = np.concatenate([keys, wgt[:, :, None]], axis=2)
    want = ts.tree_weights_numpy(full, res["trees"], mask, splits, res["breaks"], res["count"], coef, dtype=np.float64)
    got = ts.tree_weights([], b, res, coef, weights=wgt, acc=True)
    np.testing.assert_array_equal(wc.bits64(got["acc"]), wc.bits64(want))
    with pytest.raises(ValueError, match="no models"):               # a level that is read needs the weight
        ts.tree_weights([], b, res, coef)
    coef[0] = 0.0                                                    # no level that is read uses it: none is needed
    want = ts.tree_weights_numpy(full, res["trees"], mask, splits, res["breaks"], res["count"], coef, dtype=np.float64)
    np.testing.assert_array_equal(wc.bits64(ts.tree_weights([], b, res, coef, acc=True)["acc"]), wc.bits64(want))
    assert (wc.bits64(want)[mask] != 0).any()


# ---- the evaluator's flag -----------------------------------------------------------------------------
def _ckpts():
    return [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]


def test_cli_flag(monkeypatch):
    a = ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1"])
    assert a.prune_metrics is False and a.prune_weights_out is None
    assert not any(k.startswith("prune") for k in ens._extra_kwargs(a))
    trees = ["--tree_chars", "0,1", "--tree_depth", "2"]
    with pytest.raises(SystemExit):
        ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--prune_metrics"])
    with pytest.raises(SystemExit):
        ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--prune_metrics", *trees])
    with pytest.raises(SystemExit):
        ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--tree_prune", "--prune_weights_out", "w.npz", *trees])
    with pytest.raises(ValueError, match="prune_metrics needs"):
        ens.evaluate_ensemble(["c1"], "d", tree_chars="0,1", tree_depth=2, prune_metrics=True)
    seen = {}
    monkeypatch.setattr(ens, "evaluate_ensemble", lambda *args, **kw: seen.update(kw) or "ret")
    assert ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--tree_prune", *trees]) == "ret"
    assert "prune_metrics" not in seen and "prune_weights_out" not in seen
    assert ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--tree_prune", "--prune_metrics", "--prune_weights_out", "w.npz",
                     *trees]) == "ret"
    assert seen["prune_metrics"] is True and seen["prune_weights_out"] == "w.npz" and seen["tree_prune"] is True
    from src import evaluate_ensemble as cli
    assert cli.main is ens.main


def test_evaluate_ensemble_prints_the_pruned_metrics(shipped_data, tmp_path, capsys):
    kw = dict(device="cpu", verbose=True, tree_chars="0,1", tree_depth=2, tree_prune=True, prune_max_assets=8, prune_grid="2x2x6",
              paper=True)
    off_json, on_json, wout = tmp_path / "off.json", tmp_path / "on.json", tmp_path / "w.npz"
    base = ens.evaluate_ensemble(_ckpts(), shipped_data, prune_out=str(off_json), **kw)
    off_text = capsys.readouterr().out
    got = ens.evaluate_ensemble(_ckpts(), shipped_data, prune_out=str(on_json), prune_metrics=True, prune_weights_out=str(wout), **kw)
    on_text = capsys.readouterr().out
    # without the flag: no new line, no new key
    assert "STOCK-LEVEL WEIGHTS" not in off_text and "tree_prune_metrics" not in base
    assert "tree_prune_metrics" not in json.loads(off_json.read_text())
    # with it: the run's output is the flag-off output with the new block put in after the PRUNED TREES block
    bar = "=" * 70
    head = bar + "\nPRUNED TREES: STOCK-LEVEL WEIGHTS"
    i0 = on_text.index(head)
    i1 = on_text.index(f"  Saved: {on_json}")
    block = on_text[i0:i1]
    stripped = (on_text[:i0] + on_text[i1:]).replace(str(on_json), str(off_json))
    seconds = re.compile(r"\d+\.\d+ s\b")                                # (no timing is printed today; kept exact otherwise)
    assert seconds.sub("", stripped) == seconds.sub("", off_text)
    assert set(got) == set(base) | {"tree_prune_metrics"}
    for k in ("train_sharpe", "valid_sharpe", "test_sharpe", "individual_sharpes"):
        assert got[k] == base[k]
    np.testing.assert_array_equal(got["tree_prune"]["theta"], base["tree_prune"]["theta"])
    pm, pr = got["tree_prune_metrics"], got["tree_prune"]
    for s in tp.SPLITS:
        assert abs(pm[s + "_sharpe"] - pr[s + "_sharpe"]) < 1e-5
        assert f"{pm[s + '_sharpe']:8.4f}" in block
    assert f"{pm['self_check']:.3e}" in block and f"{pm['ev']:8.4f}" in block
    # the run has the ensemble's paper metrics: its row stands next to the pruned trees'
    assert f"{'Ensemble':14s} {got['paper_metrics']['test']['ev']:8.4f}" in block
    d = json.loads(on_json.read_text())
    assert d["tree_prune_metrics"]["xs_r2"] == pm["xs_r2"] and d["valid_sharpe"] == pr["valid_sharpe"]
    z = np.load(wout)
    assert set(z.files) == set(tp.SPLITS) and z["test"].dtype == np.float32 and z["test"].ndim == 2
    # the self-check is the float32 rounding of w: 2^-24 sum_i |w R| per period (the float64 orders are far below it)
    lim = 0.0
    for s, ds in zip(tp.SPLITS, ens.load_splits(shipped_data)):
        b = ds.get_full_batch()
        r, m = b["returns"].numpy().astype(np.float64), b["mask"].numpy().astype(bool)
        assert z[s].shape == m.shape and (z[s][~m] == 0).all()
        lim = max(lim, float((np.abs(z[s] * r) * m).sum(axis=1).max()))
    assert pm["self_check"] <= 2.0 ** -23 * lim

"""Pruning the tree portfolios (``analysis.tree_prune``) on the CPU: the jump form of ``en_paths_numpy``
against the loop of the definition, the KKT conditions at every converged point, the behaviour along a
path (first point, ``diag <= 0``, ``max_assets``), the argument checks, ``prune_trees`` on a small
planted panel and the evaluator's flag."""
import json
import os

import numpy as np
import pytest

import golden_cases as gc
import prune_cases as pc
from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
from deeplearninginassetpricing_paperreplication_amd.analysis.portfolio import sharpe_ddof0


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["n1", "n13", "rank_deficient", "zero_diagonal", "max_assets"])
def test_jump_form_is_the_loop(name):
    c, o = pc.case(name), pc.oracle(name)
    for p in range(c["b"].shape[0] if c["b"].shape[1] < 20 or c["max_assets"] else 1):
        th, sw, nz, up = tp.en_path_loop(c["A"][c["a_of"][p]], c["b"][p], c["l1s"][p], c["l2"][p], c["max_sweeps"], c["max_assets"])
        np.testing.assert_array_equal(_bits(th), _bits(o["theta"][p]))
        np.testing.assert_array_equal(sw, o["sweeps"][p])
        np.testing.assert_array_equal(nz, o["nnz"][p])
        np.testing.assert_array_equal(up, o["updates"][p])
    assert o["theta"].dtype == np.float64 and o["sweeps"].dtype == np.int32 and o["nnz"].dtype == np.int32


@pytest.mark.parametrize("name", ["n1", "n13", "n64", "zero_diagonal", "max_assets", "two_matrices"])
def test_converged_points_satisfy_kkt(name):
    """r = b - M th - l2 th; at a non-zero coordinate |r_j - l1 sign(th_j)| <= bound_j, at a zero one
    |r_j| <= l1 + bound_j, bound_j = delta sum_m |M_jm| + 64 eps (|b_j| + sum_m |M_jm th_m|) with delta
    the stopping threshold: a coordinate was exact at its own update and the later updates of the last
    sweep moved g_j by at most delta sum_m |M_jm|."""
    c = pc.two_matrix_case() if name == "two_matrices" else pc.case(name)
    o = pc.oracle(name)
    eps = np.finfo(np.float64).eps
    checked = 0
    for p in range(c["b"].shape[0]):
        M, b, l2 = c["A"][c["a_of"][p]], c["b"][p], c["l2"][p]
        live = np.diagonal(M) + l2 > 0                       # (a coordinate with diag <= 0 is held at 0, not optimised)
        for k in range(c["l1s"].shape[1]):
            if not 0 < o["sweeps"][p, k] < c["max_sweeps"]:
                continue
            th, l1 = o["theta"][p, k], c["l1s"][p, k]
            r = b - M @ th - l2 * th
            delta = tp.EN_TOL * max(1.0, np.abs(th).max())
            bound = delta * np.abs(M).sum(axis=1) + 64 * eps * (np.abs(b) + np.abs(M * th[None, :]).sum(axis=1))
            nzc = th != 0
            assert (np.abs(r - l1 * np.sign(th))[nzc & live] <= bound[nzc & live]).all(), (name, p, k)
            assert (np.abs(r)[~nzc & live] <= l1 + bound[~nzc & live]).all(), (name, p, k)
            checked += 1
    assert checked >= 2


def test_path_behaviour():
    c, o = pc.case("n70"), pc.oracle("n70")
    # the first point, l1 = max |b|: nothing enters, one sweep
    assert (o["sweeps"][:, 0] == 1).all() and (o["nnz"][:, 0] == 0).all() and not o["theta"][:, 0].any()
    # the path opens up as l1 falls and every point is computed without max_assets
    assert (o["sweeps"] >= 1).all() and (np.diff(o["nnz"], axis=1)[:, :3] >= 0).all() and o["nnz"][:, -1].min() > 40
    assert (o["nnz"] == (o["theta"] != 0).sum(axis=2)).all()
    # the cap: l2 = 0 with T < n
    r = pc.oracle("rank_deficient")
    assert (r["sweeps"][:, 1:] == pc.MAX_SWEEPS).all()


def test_nonpositive_diagonal_stays_zero():
    c, o = pc.case("zero_diagonal"), pc.oracle("zero_diagonal")
    zd = list(c["zero_diag"])
    assert (np.diagonal(c["A"][0])[zd] == 0).all() and c["l2"][0] == 0 and (c["b"][0][zd] != 0).all()
    assert not o["theta"][0][:, zd].any() and o["nnz"][0, -1] > 0          # diag = 0: held at 0
    assert o["theta"][1][-1, zd].all()                                       # diag = l2 > 0: it moves
    A = np.array([[[-1.0, 0.0], [0.0, 1.0]]])
    got = tp.en_paths_numpy(A, [0], [[1.0, 1.0]], [[0.5, 0.1]], [0.25])
    np.testing.assert_array_equal(got["theta"][0], [[0.0, 0.5 / 1.25], [0.0, 0.9 / 1.25]])
    np.testing.assert_array_equal(got["nnz"], [[1, 1]])


def test_max_assets_ends_the_path():
    c, o = pc.case("max_assets"), pc.oracle("max_assets")
    A, a_of, b, l1s, l2 = pc.call_args(c)
    full = tp.en_paths_numpy(A, a_of, b, l1s[:, :4], l2, max_sweeps=c["max_sweeps"])      # the first points without the limit
    for p in range(c["b"].shape[0]):
        over = np.flatnonzero(full["nnz"][p] > c["max_assets"])
        assert over.size and over[0] + 1 < 4
        last = over[0]                                       # the first point above the limit is kept, the rest is not run
        np.testing.assert_array_equal(_bits(o["theta"][p, :last + 1]), _bits(full["theta"][p, :last + 1]))
        np.testing.assert_array_equal(o["sweeps"][p, :last + 1], full["sweeps"][p, :last + 1])
        assert o["nnz"][p, last] > c["max_assets"] and (o["nnz"][p, :last] <= c["max_assets"]).all()
        assert not o["sweeps"][p, last + 1:].any() and not o["nnz"][p, last + 1:].any() and not o["theta"][p, last + 1:].any()
        assert (_bits(o["theta"][p, last + 1:]) == 0).all()


def test_argument_checks():
    c = pc.case("n13")
    A, a_of, b, l1s, l2 = pc.call_args(c)
    bad = A.copy(); bad[0, 2, 5] = np.nextafter(bad[0, 2, 5], 1.0)
    with pytest.raises(ValueError, match="symmetric"):
        tp.en_paths_numpy(bad, a_of, b, l1s, l2)
    bad = b.copy(); bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        tp.en_paths_numpy(A, a_of, bad, l1s, l2)
    bad = A.copy(); bad[0, 4, 4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        tp.en_paths_numpy(bad, a_of, b, l1s, l2)
    with pytest.raises(ValueError, match="non-negative"):
        tp.en_paths_numpy(A, a_of, b, -l1s, l2)
    with pytest.raises(ValueError, match="non-negative"):
        tp.en_paths_numpy(A, a_of, b, l1s, l2 - 1.0)
    with pytest.raises(ValueError, match="a_of"):
        tp.en_paths_numpy(A, a_of + 1, b, l1s, l2)
    with pytest.raises(ValueError):
        tp.en_paths_numpy(A, a_of, b[:, :5], l1s, l2)
    with pytest.raises(ValueError):
        tp.en_paths_numpy(A, a_of, b, l1s, l2, max_sweeps=0)
    got = tp.en_paths(A, a_of, b, l1s, l2, max_sweeps=c["max_sweeps"], device="cpu")      # the dispatcher on the CPU
    np.testing.assert_array_equal(_bits(got["theta"]), _bits(pc.oracle("n13")["theta"]))


def test_moments_and_node_returns():
    res = pc.planted_tree_results()["train"]
    R, un = tp.node_returns(res)
    R1, _ = tp.node_returns(res, depth_weight=False)
    assert len(un["nodes"]) == 1 + 4 + 16 and R.shape == (40, 21) and un["nodes"][0] == (0, 0)
    lev = np.asarray(un["levels"])
    np.testing.assert_array_equal(R, R1 * (1.0 / np.sqrt(np.array([1.0, 2.0, 4.0])[lev]))[None, :])
    for a in (0, 3, 20):                                     # the root, a level-1 and a level-2 node
        tr, nd = un["nodes"][a]
        np.testing.assert_array_equal(R1[:, a], np.nan_to_num(res["returns"][:, tr, nd].astype(np.float64)))
    mu, S = tp.mv_moments(R)
    np.testing.assert_array_equal(_bits(S), _bits(S.T))
    np.testing.assert_allclose(S, np.cov(R.T, ddof=0), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(mu, R.mean(axis=0))
    empty = dict(res, returns=np.where(np.arange(40)[:, None, None] < 3, np.nan, res["returns"]))
    assert not tp.node_returns(empty)[0][:3].any()          # an empty node counts as a return of 0


def test_prune_trees_on_the_planted_panel(tmp_path):
    by_split = pc.planted_tree_results()
    pr = tp.prune_trees(by_split, n1=8, max_assets=6, max_sweeps=pc.MAX_SWEEPS, device="cpu")
    P, n1 = 9, 8
    assert pr["nnz"].shape == (P, n1) and pr["assets"] == 21 and "gpu_ms" not in pr
    # the paths, l0-major
    R = {s: tp.node_returns(by_split[s])[0] for s in tp.SPLITS}
    mu, S = tp.mv_moments(R["train"])
    assert pr["grid_l0"] == [0.0, 0.25, 0.5] and pr["grid_l2_rel"] == [1e-3, 1e-2, 1e-1]
    np.testing.assert_array_equal(pr["grid_l2"], np.tile(np.array([1e-3, 1e-2, 1e-1]) * np.trace(S) / 21, 3))
    np.testing.assert_array_equal(pr["grid_l1"][4], np.abs(mu + 0.25 * mu.mean()).max() * 10.0 ** (-np.linspace(0.0, 3.0, 8)))
    # the selection: the first argmax of the validation Sharpe over the eligible points
    elig = (pr["sweeps"] > 0) & (pr["nnz"] >= 1) & (pr["nnz"] <= 6)
    np.testing.assert_array_equal(pr["eligible"], elig)
    assert elig.any() and not elig.all()
    sel = int(np.argmax(np.where(elig, pr["sharpe"]["valid"], -np.inf)))
    assert (pr["path"], pr["point"]) == divmod(sel, n1)
    assert pr["valid_sharpe"] == np.nanmax(pr["sharpe"]["valid"][elig])
    assert (pr["l0"], pr["l2_rel"]) == ((0.0, 0.25, 0.5)[pr["path"] // 3], (1e-3, 1e-2, 1e-1)[pr["path"] % 3])
    th = pr["theta"]
    assert 1 <= np.count_nonzero(th) == pr["nnz"][pr["path"], pr["point"]] <= 6
    for s in tp.SPLITS:
        assert pr[s + "_sharpe"] == sharpe_ddof0(R[s] @ th) == pr["sharpe"][s][pr["path"], pr["point"]]
    assert np.isnan(pr["sharpe"]["valid"][~pr["computed"]]).all() and np.isfinite(pr["sharpe"]["valid"][pr["computed"]]).all()
    # max_assets ended every path that went above it
    for p in range(P):
        over = np.flatnonzero(pr["nnz"][p] > 6)
        assert over.size <= 1 and (not over.size or not pr["sweeps"][p, over[0] + 1:].any())
    # the selected nodes, and the depth weights in the assets
    un = ts.unique_nodes(by_split["train"]["trees"], by_split["train"]["splits"])
    assert [(tr, nd) for tr, nd, *_ in pr["nodes"]] == [un["nodes"][a] for a in np.flatnonzero(th)]
    for tr, nd, path, lev, w in pr["nodes"]:
        assert len(path) == lev and w == th[un["nodes"].index((tr, nd))]
    plain = tp.prune_trees(by_split, n1=8, max_assets=6, max_sweeps=pc.MAX_SWEEPS, device="cpu", depth_weight=False)
    assert not np.array_equal(plain["grid_l1"], pr["grid_l1"]) and plain["depth_weight"] is False
    # the report and the JSON form
    lines = tp.format_pruned(pr, gan={"train_sharpe": 0.5, "valid_sharpe": 0.25, "test_sharpe": 0.125})
    assert any(l.lstrip().startswith("Pruned trees") for l in lines) and any(l.lstrip().startswith("Ensemble") for l in lines)
    assert sum("level" in l for l in lines) == len(pr["nodes"])
    out = tmp_path / "pruned.json"
    out.write_text(json.dumps(tp.pruned_to_json(pr), allow_nan=False))
    d = json.loads(out.read_text())
    assert d["theta"] == th.tolist() and d["nnz"] == pr["nnz"].tolist() and d["path"] == pr["path"]
    assert d["valid_sharpe"] == pr["valid_sharpe"] and len(d["nodes"]) == len(pr["nodes"])
    assert d["nodes"][0]["weight"] == pr["nodes"][0][4] and d["nodes"][0]["path"] == [list(x) for x in pr["nodes"][0][2]]
    assert d["sharpe"]["test"][pr["path"]][pr["point"]] == pr["test_sharpe"]
    # nothing eligible
    with pytest.raises(ValueError, match="no computed point"):
        tp.prune_trees(by_split, n1=1, max_assets=6, device="cpu")
    with pytest.raises(ValueError, match="split"):
        tp.prune_trees({"train": by_split["train"]}, device="cpu")


def test_grid_parsing():
    assert tp.parse_prune_grid("3x3x16") == (3, 3, 16) and tp.parse_prune_grid("1x2x5") == (1, 2, 5)
    for bad in ("3x3", "4x3x16", "3x0x16", "axbxc", "3x3x0"):
        with pytest.raises(ValueError):
            tp.parse_prune_grid(bad)


def _ckpts():
    return [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]


def test_cli_flag(monkeypatch):
    a = ens._parser().parse_args(["--data_dir", "d", "--checkpoint_dirs", "c1"])
    assert a.tree_prune is False and a.prune_max_assets == 40 and a.prune_grid == "3x3x16" and a.prune_out is None
    assert not any(k.startswith("prune") or k == "tree_prune" for k in ens._extra_kwargs(a))
    # the flag without trees
    with pytest.raises(SystemExit):
        ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--tree_prune"])
    with pytest.raises(ValueError, match="tree_prune needs"):
        ens.evaluate_ensemble(["c1"], "d", tree_prune=True)
    seen = {}
    monkeypatch.setattr(ens, "evaluate_ensemble", lambda *args, **kw: seen.update(kw) or "ret")
    assert ens.main(["--data_dir", "d", "--checkpoint_dirs", "c1", "--tree_chars", "0,1,2", "--tree_depth", "4", "--tree_prune",
                     "--prune_max_assets", "12", "--prune_grid", "2x3x8", "--prune_out", "p.json"]) == "ret"
    assert seen["tree_prune"] is True and seen["prune_max_assets"] == 12 and seen["prune_grid"] == "2x3x8"
    assert seen["prune_out"] == "p.json" and seen["tree_chars"] == "0,1,2"


def test_evaluate_ensemble_prunes_the_trees(shipped_data, tmp_path, capsys):
    kw = dict(device="cpu", verbose=True, tree_chars="0,1", tree_depth=2)
    base = ens.evaluate_ensemble(_ckpts(), shipped_data, **kw)
    plain_text = capsys.readouterr().out
    assert "PRUNED TREES" not in plain_text and "tree_prune" not in base
    out = tmp_path / "pruned.json"
    got = ens.evaluate_ensemble(_ckpts(), shipped_data, tree_prune=True, prune_max_assets=8, prune_grid="2x2x6",
                                prune_out=str(out), **kw)
    text = capsys.readouterr().out
    head = "PRUNED TREES (elastic-net mean-variance SDF on the tree nodes, at most 8)"
    assert head in text and text[:text.index("=" * 70 + "\n" + head)] == plain_text
    assert set(got) == set(base) | {"tree_prune"}
    for k in ("train_sharpe", "valid_sharpe", "test_sharpe", "individual_sharpes"):
        assert got[k] == base[k]
    pr = got["tree_prune"]
    assert pr["nnz"].shape == (4, 6) and pr["assets"] == 1 + 4 + 16 and 1 <= len(pr["nodes"]) <= 8
    assert all(np.isfinite(pr[s + "_sharpe"]) for s in tp.SPLITS)
    assert f"{pr['test_sharpe']:8.4f}" in text and f"{base['test_sharpe']:8.4f}" in text
    d = json.loads(out.read_text())
    assert d["valid_sharpe"] == pr["valid_sharpe"] and len(d["nodes"]) == len(pr["nodes"])

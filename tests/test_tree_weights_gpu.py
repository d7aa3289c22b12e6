"""``k_qtree_weight`` (``Engine.tree_weights``, ``csrc/k_qtree_weight.hip``) on a real MI355X against
``tree_sorts.tree_weights_numpy``: every comparison is on the uint32 view of ``w`` and the uint64 view of
``acc_out``, without a tolerance. The oracle runs on the keys the engine holds (bf16-rounded
characteristics for a bf16 panel, fp32 extra keys) with the ``breaks`` / ``count`` that
``Engine.tree_sorted_portfolios`` returned on the same engine. Both outputs are prefilled with a sentinel
that has to survive at every invalid cell. Panels: ``weight_cases.gpu_panel``. Agreement counts:
profiles/tree_weights_accuracy.txt."""
import itertools
import math

import numpy as np
import pytest
import torch

import weight_cases as wc
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

SENT32, SENT64 = 0x7FC12345, 0x7FF8123456789ABC          # NaN payloads no result can take


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


def _spec(F):
    return AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).spec


_ENGINES, _SORTS = {}, {}


def _engine(name, precision):
    """One engine per (panel, precision), with the panel's extra keys on the device."""
    key = (name, precision)
    if key not in _ENGINES:
        from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
        b, extra = wc.gpu_panel(name)
        eng = GANEngine(_spec(b["individual_features"].shape[2]), 1, max_epochs=4, precision=precision)
        eng.set_data(b)
        if name == "W":
            assert int(eng.desc["wide"]) == 1
        ek = torch.as_tensor(extra).cuda().contiguous() if extra is not None else None
        torch.cuda.synchronize()
        _ENGINES[key] = (eng, ek)
    return _ENGINES[key]


def _sort(name, precision, trees, splits):
    """``breaks`` and ``count`` of the engine's own tree sort."""
    key = (name, precision, tuple(trees), tuple(splits))
    if key not in _SORTS:
        eng, ek = _engine(name, precision)
        r = eng.eng.tree_sorted_portfolios(0, [list(tr) for tr in trees], list(splits), ek.data_ptr() if ek is not None else 0,
                                           0 if ek is None else ek.shape[0], 0, 0)
        eng.eng.sync()
        _SORTS[key] = (np.asarray(r["breaks"]).copy(), np.asarray(r["count"]).copy())
    return _SORTS[key]


def _oracle(name, precision, trees, splits, breaks, count, coef):
    mask = wc.gpu_panel(name)[0]["mask"].numpy()
    return ts.tree_weights_numpy(wc.engine_keys(name, precision), trees, mask, splits, breaks, count, coef, dtype=np.float64)


def _run(name, precision, trees, splits, breaks, count, coef, tpp=0, acc=True, verify=False):
    """``(w, acc, result dict)`` of one call into sentinel-filled outputs."""
    eng, ek = _engine(name, precision)
    T, N = wc.gpu_panel(name)[0]["mask"].shape
    w = torch.full((T, N), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    a = torch.full((T, N), SENT64, dtype=torch.int64, device="cuda").view(torch.float64)
    torch.cuda.synchronize()
    r = eng.eng.tree_weights(0, [list(tr) for tr in trees], list(splits), breaks, count, coef, ek.data_ptr() if ek is not None else 0,
                             0 if ek is None else ek.shape[0], w.data_ptr(), a.data_ptr() if acc else 0, tpp, verify)
    eng.eng.sync()
    return w.cpu().numpy(), a.cpu().numpy(), r


def _check(name, got_w, got_a, want, acc=True):
    """The oracle's bits at the valid cells, the sentinel everywhere else; returns the number of valid cells."""
    mask = wc.gpu_panel(name)[0]["mask"].numpy()
    gw, ga = wc.bits32(got_w), wc.bits64(got_a)
    np.testing.assert_array_equal(gw[mask], wc.bits32(want.astype(np.float32))[mask])
    assert (gw[~mask] == SENT32).all()
    if acc:
        np.testing.assert_array_equal(ga[mask], wc.bits64(want)[mask])
        assert (ga[~mask] == SENT64).all()
    else:
        assert (ga == SENT64).all()
    return int(mask.sum())


def _case(name, precision, trees, splits, coef, **kw):
    breaks, count = _sort(name, precision, trees, splits)
    want = _oracle(name, precision, trees, splits, breaks, count, coef)
    w, a, r = _run(name, precision, trees, splits, breaks, count, coef, **kw)
    n = _check(name, w, a, want, acc=kw.get("acc", True))
    print(f"{name} {precision} {splits}: {n} valid cells, all bits equal; {r['active_trees']} active trees, {r['passes']} passes, "
          f"{r['keys']} keys, {float(r['gpu_ms']):.3f} ms")
    return want, r


@pytest.mark.parametrize("splits", [(2, 2, 2), (2, 2, 2, 2, 2), (3, 3, 4), (16, 2), (6, 6)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_a_matches_numpy(precision, splits):
    trees = wc.gpu_trees(wc.KEYS_A, len(splits), 10)
    P, NN = len(trees), ts.tree_layout(splits)["nodes"]
    want, r = _case("A", precision, trees, splits, wc.dense_coef(P, NN, 21, decades=3))
    assert r["active_trees"] == P and r["passes"] == 1 and float(r["gpu_ms"]) > 0 and r["segments"] == 11
    assert len(np.unique(wc.bits64(want))) > 100                    # (the weights do differ from stock to stock)
    _, r = _case("A", precision, trees, splits, wc.sparse_coef(P, splits))
    assert r["active_trees"] == 2 and r["keys"] == len(ts.active_keys(trees, splits, wc.sparse_coef(P, splits)))


@pytest.mark.parametrize("splits", [(2, 2, 2, 2), (3, 3, 4), (2, 16), (5, 5)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_b_row_segments_and_mixed_key_widths(precision, splits):
    D = len(splits)
    # the tie-free extra key on every level, the rotations, then bf16 and fp32 keys in every order
    trees = list(dict.fromkeys([(5,) * D] + wc.gpu_trees(wc.KEYS_B, D, 6) + list(itertools.product((1, 5), repeat=D))[:8]
                               + list(itertools.product((6, 2), repeat=D))[:4]))
    P, NN = len(trees), ts.tree_layout(splits)["nodes"]
    assert P > 16 or D == 2                                          # more than one pass at the default
    _, r = _case("B", precision, trees, splits, wc.dense_coef(P, NN, 22, decades=3))
    assert r["segments"] == 3 * 11 and r["passes"] == -(-P // 16) and r["keys"] == 4
    _case("B", precision, trees, splits, wc.sparse_coef(P, splits), acc=False)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_path_engine(precision):
    trees = [(0, 129, 64), (128, 64, 0), (77, 77, 77), (129, 1, 128)]
    for splits in ((2, 2, 2), (3, 3, 4)):
        NN = ts.tree_layout(splits)["nodes"]
        _case("W", precision, trees, splits, wc.dense_coef(4, NN, 23, decades=2))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_trees_per_pass_and_tree_order_change_no_bit(precision):
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    splits = (2, 3, 3)
    trees = wc.gpu_trees(wc.KEYS_A, 3, 10)
    P, NN = len(trees), ts.tree_layout(splits)["nodes"]
    coef = wc.dense_coef(P, NN, 24, decades=3)
    coef[4] = 0.0                                                    # one tree drops out of the call
    breaks, count = _sort("A", precision, trees, splits)
    want = _oracle("A", precision, trees, splits, breaks, count, coef)
    for tpp in (1, 3, 0, nat.QTREE_WEIGHT_MAX_TPP):
        w, a, r = _run("A", precision, trees, splits, breaks, count, coef, tpp=tpp)
        _check("A", w, a, want)
        assert r["active_trees"] == P - 1 and r["passes"] == -(-(P - 1) // (tpp or nat.QTREE_WEIGHT_DEFAULT_TPP))
    # the tree list reordered: the bits of the oracle of the order passed (another order of the additions)
    perm = [7, 2, 9, 0, 5, 4, 1, 8, 3, 6]
    ptrees = [trees[p] for p in perm]
    pb, pc_, pcoef = np.ascontiguousarray(breaks[:, perm]), np.ascontiguousarray(count[:, perm]), np.ascontiguousarray(coef[perm])
    pwant = _oracle("A", precision, ptrees, splits, pb, pc_, pcoef)
    assert (wc.bits64(pwant) != wc.bits64(want)).any()
    for tpp in (1, 3, 0):
        w, a, _ = _run("A", precision, ptrees, splits, pb, pc_, pcoef, tpp=tpp)
        _check("A", w, a, pwant)
    # ... and undone on the host: the first call again
    inv = np.argsort(perm)
    w, a, _ = _run("A", precision, [ptrees[p] for p in inv], splits, np.ascontiguousarray(pb[:, inv]),
                   np.ascontiguousarray(pc_[:, inv]), np.ascontiguousarray(pcoef[inv]), tpp=3)
    _check("A", w, a, want)


def test_inputs_are_not_written_and_zero_coef_launches_nothing():
    splits = (2, 2, 2, 2)
    trees = wc.gpu_trees(wc.KEYS_B, 4, 7)
    P, NN = len(trees), ts.tree_layout(splits)["nodes"]
    breaks, count = _sort("B", "bf16", trees, splits)
    coef = wc.dense_coef(P, NN, 25)
    _, ek = _engine("B", "bf16")
    keep = [breaks.copy(), count.copy(), coef.copy(), ek.clone()]
    want = _oracle("B", "bf16", trees, splits, breaks, count, coef)
    # verify_inputs: the engine reads its device copies of breaks, count and coef back after the launch and
    # compares them with what it uploaded; the extra keys are the caller's device tensor
    w, a, r = _run("B", "bf16", trees, splits, breaks, count, coef, verify=True)
    _check("B", w, a, want)
    assert r["inputs_unchanged"] is True
    assert "inputs_unchanged" not in _run("B", "bf16", trees, splits, breaks, count, coef)[2]
    assert breaks.tobytes() == keep[0].tobytes() and count.tobytes() == keep[1].tobytes() and coef.tobytes() == keep[2].tobytes()
    assert torch.equal(ek.view(torch.int32), keep[3].view(torch.int32))
    # the sort's own tables on the device side of the engine are untouched too: sorting again gives the same bytes
    _SORTS.clear()
    b2, c2 = _sort("B", "bf16", trees, splits)
    assert b2.tobytes() == breaks.tobytes() and c2.tobytes() == count.tobytes()
    # all coefficients zero (or -0.0): nothing is launched, nothing is written
    for z in (np.zeros((P, NN)), np.full((P, NN), -0.0)):
        w, a, r = _run("B", "bf16", trees, splits, breaks, count, z)
        assert (wc.bits32(w) == SENT32).all() and (wc.bits64(a) == SENT64).all()
        assert r["active_trees"] == 0 and r["passes"] == 0 and float(r["gpu_ms"]) == 0.0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_one_hot_leaves_give_one_over_the_leaf_size(precision):
    splits = (3, 3, 4)
    trees = wc.gpu_trees(wc.KEYS_A, 3, 10)
    lay = ts.tree_layout(splits)
    first = lay["level_offsets"][lay["depth"]]
    breaks, count = _sort("A", precision, trees, splits)
    mask = wc.gpu_panel("A")[0]["mask"].numpy()
    for p in (0, 3, 9):                                              # (0: the constant first key, most leaves empty)
        w, a, r = _run("A", precision, trees, splits, breaks, count, wc.one_hot_leaves(len(trees), splits, p))
        assert r["active_trees"] == 1
        for t in range(mask.shape[0]):
            leaves = count[t, p, first:]
            sizes = sorted(set(int(m) for m in leaves if m > 0))
            assert sorted(set(w[t][mask[t]].tolist())) == sorted(float(np.float32(1.0 / m)) for m in sizes)
            for m in sizes:                                          # a leaf of m rows: m stocks carry 1 / m
                assert int((w[t][mask[t]] == np.float32(1.0 / m)).sum()) == m * int((leaves == m).sum())
            # the exactly rounded sum of the period's acc: every non-empty leaf adds up to one
            assert math.fsum(a[t][mask[t]].tolist()) == float((leaves > 0).sum())
    assert (count[2, :, first:] == 0).any() and (count[5] == 0).all()


def test_a_call_with_the_most_keys_and_trees_per_pass():
    """32 distinct keys and 32 trees a pass: the largest LDS image of the kernel."""
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    splits = (2, 2, 2, 2, 2)
    trees = [tuple((5 * s + k) % 32 for k in range(5)) for s in range(34)]
    assert len({c for tr in trees for c in tr}) == nat.QTREE_WEIGHT_MAX_KEYS == 32
    NN = ts.tree_layout(splits)["nodes"]
    _, r = _case("A", "bf16", trees, splits, wc.dense_coef(len(trees), NN, 26), tpp=nat.QTREE_WEIGHT_MAX_TPP)
    assert r["keys"] == 32 and r["passes"] == 2


def test_pruned_weights_on_the_gpu_are_the_cpu_bits():
    """fp32 keys: both paths see the same numbers, so the walk and every sum are the same."""
    pr, by_split, batches = wc.planted_case()
    torch.manual_seed(5)
    models = [AssetPricingGAN(default_cli_config(8, 2, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).eval()]
    cpu = tp.pruned_weights(pr, by_split, batches, models, device="cpu")
    gpu = tp.pruned_weights(pr, by_split, batches, models, device="cuda", precision="fp32")
    for s in tp.SPLITS:
        np.testing.assert_array_equal(wc.bits32(gpu[s]), wc.bits32(cpu[s]))
        assert (wc.bits32(gpu[s]) != 0).any()
    res, b = by_split["test"], batches["test"]
    out = ts.tree_weights(models, b, res, tp.node_coefficients(pr, res), device="cuda", precision="fp32", acc=True, trees_per_pass=1)
    ref = ts.tree_weights(models, b, res, tp.node_coefficients(pr, res), device="cpu", acc=True)
    np.testing.assert_array_equal(wc.bits64(out["acc"]), wc.bits64(ref["acc"]))
    assert out["gpu_ms"] > 0 and out["passes"] == out["active_trees"] >= 1


def test_limits_and_the_fallback(capsys):
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    # the limits the README states
    assert nat.QTREE_WEIGHT_MAX_KEYS == ts.MAX_WEIGHT_KEYS == 32 and nat.QTREE_WEIGHT_MAX_TREES == ts.MAX_TREES == 4096
    assert nat.QTREE_WEIGHT_SEG == 256 and nat.QTREE_WEIGHT_DEFAULT_TPP == 16 and nat.QTREE_WEIGHT_MAX_TPP == 32
    assert nat.QTREE_MAX_D == ts.MAX_DEPTH == 5 and nat.QTREE_MAX_LEAVES == ts.MAX_LEAVES == 36
    ok = nat.qtree_weight_supported
    assert ok([2] * 5, 4096, 65535, 32) and ok([6, 6], 1, 1, 0) and ok([16, 2], 0, 0, 16)
    assert not ok([2] * 5, 4096, 65535, 33) and not ok([2] * 5, 4097, 1, 1) and not ok([2] * 5, 1, 65536, 1)
    assert not ok([2] * 6, 1, 1, 1) and not ok([6, 7], 1, 1, 1) and not ok([17, 2], 1, 1, 1) and not ok([], 1, 1, 1)
    # 33 distinct keys: the Python layer says so and runs numpy (fp32 keys on both sides)
    b, _ = wc.gpu_panel("A")
    torch.manual_seed(6)
    models = [AssetPricingGAN(default_cli_config(8, 46, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).eval()]
    trees = [(3 * s, 3 * s + 1, 3 * s + 2) for s in range(11)]
    res = ts.tree_sorted_portfolios(models, b, trees, splits=(2, 2, 2), device="cuda", precision="fp32",
                                    weights=np.zeros(b["mask"].shape, np.float32))
    coef = wc.dense_coef(11, 15, 27)
    capsys.readouterr()
    got = ts.tree_weights(models, b, res, coef, device="cuda", precision="fp32")
    note = capsys.readouterr().out
    assert "33 distinct keys" in note and "using the numpy path" in note and "gpu_ms" not in got
    want = ts.tree_weights(models, b, res, coef, device="cpu")
    np.testing.assert_array_equal(wc.bits32(got["w"]), wc.bits32(want["w"]))
    # one tree less: the kernel, the same bits
    coef[10] = 0.0
    capsys.readouterr()
    got = ts.tree_weights(models, b, res, coef, device="cuda", precision="fp32")
    assert "numpy path" not in capsys.readouterr().out and got["gpu_ms"] > 0 and got["active_trees"] == 10
    np.testing.assert_array_equal(wc.bits32(got["w"]), wc.bits32(ts.tree_weights(models, b, res, coef, device="cpu")["w"]))
    # a bf16 sort: the fallback walks the bf16-rounded characteristics, the keys the sort saw
    coef = wc.dense_coef(11, 15, 27)
    res16 = ts.tree_sorted_portfolios(models, b, trees, splits=(2, 2, 2), device="cuda", weights=np.zeros(b["mask"].shape, np.float32))
    capsys.readouterr()
    got = ts.tree_weights(models, b, res16, coef, device="cuda")
    assert "using the numpy path" in capsys.readouterr().out
    mask = b["mask"].numpy()
    want = ts.tree_weights_numpy(wc.engine_keys("A", "bf16"), trees, mask, (2, 2, 2), res16["breaks"], res16["count"], coef)
    np.testing.assert_array_equal(wc.bits32(got["w"]), wc.bits32(want))
    try:                                                             # (the unrounded keys do walk elsewhere on this panel)
        other = ts.tree_weights_numpy(wc.engine_keys("A", "fp32"), trees, mask, (2, 2, 2), res16["breaks"], res16["count"], coef)
        assert (wc.bits32(other) != wc.bits32(want)).any()
    except ValueError:
        pass


def test_python_layer_with_trees_that_sort_on_the_weight():
    """``tree_weights`` / ``pruned_weights`` on trees that name ``weight``: read (an active level), named only below
    the tree's deepest non-zero level, named by a tree without a coefficient, and a tree of which only the root
    is selected. fp32 keys, one ensemble weight handed to both devices: the CPU result bit for bit."""
    from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp
    b, _ = wc.gpu_panel("A")
    models = []
    for g in range(2):
        torch.manual_seed(200 + g)
        models.append(AssetPricingGAN(default_cli_config(8, 46, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).eval())
    wgt = sp._gpu_weights(models, b).cpu().numpy()
    trees, splits = [("weight", 3, 4), (3, 4, "weight"), (46, 46, 46), (7, "weight", 9), (1, 2, 3)], (2, 3, 3)
    res = ts.tree_sorted_portfolios(models, b, trees, splits=splits, device="cuda", precision="fp32", weights=wgt)
    lay = ts.tree_layout(splits)
    off = lay["level_offsets"]
    coef = wc.dense_coef(5, lay["nodes"], 31, decades=2)
    coef[1, off[3]:] = 0.0                                           # tree 1: the weight is below its deepest non-zero level
    coef[2] = 0.0                                                    # tree 2: no coefficient at all
    coef[3, 1:] = 0.0                                                # tree 3: the root only
    kw = dict(precision="fp32", acc=True)
    for read in (True, False):
        if not read:
            coef[0] = 0.0                                            # now no level that is read uses the weight
        assert (46 in ts.active_keys(res["trees"], splits, coef)) is read
        cpu = ts.tree_weights(models, b, res, coef, device="cpu", weights=wgt, acc=True)
        for given in (wgt, None) if not read else (wgt,):            # (unread: no weight has to be handed over)
            gpu = ts.tree_weights(models, b, res, coef, device="cuda", weights=given, **kw)
            np.testing.assert_array_equal(wc.bits64(gpu["acc"]), wc.bits64(cpu["acc"]))
            np.testing.assert_array_equal(wc.bits32(gpu["w"]), wc.bits32(cpu["w"]))
            assert gpu["active_trees"] == (4 if read else 3) and (wc.bits32(gpu["w"]) != 0).any()
    # the pruned SDF on the same trees: the root, a level-1 node of the weight tree and a leaf below a weight level
    un = ts.unique_nodes(res["trees"], splits)
    theta = np.zeros(len(un["nodes"]))
    for node, v in (((0, 0), 0.5), ((0, off[1] + 1), -1.5), ((3, off[3] + 4), 2.0)):
        theta[un["nodes"].index(node)] = v
    for sel in (theta, np.where(np.arange(theta.size) == un["nodes"].index((0, 0)), theta, 0.0)):   # (then the root alone)
        pr = {"theta": sel, "depth_weight": True}
        c = tp.pruned_weights(pr, {"test": res}, {"test": b}, models, device="cpu", weights={"test": wgt})
        g = tp.pruned_weights(pr, {"test": res}, {"test": b}, models, device="cuda", precision="fp32", weights={"test": wgt})
        np.testing.assert_array_equal(wc.bits32(g["test"]), wc.bits32(c["test"]))
        assert (wc.bits32(g["test"]) != 0).any()


def test_bad_arguments():
    eng, _ = _engine("A", "bf16")
    e = eng.eng
    trees, splits = [(0, 1), (2, 3)], [2, 3]
    breaks, count = _sort("A", "bf16", [tuple(t) for t in trees], tuple(splits))
    coef = wc.dense_coef(2, 9, 28)
    w = torch.zeros(12, 150, device="cuda")
    torch.cuda.synchronize()
    good = dict(s=0, trees=trees, splits=splits, breaks=breaks, count=count, coef=coef, w_out=w.data_ptr())
    assert e.tree_weights(**good)["active_trees"] == 2
    for kw in (dict(splits=[2, 1]), dict(splits=[6, 7]), dict(splits=[]), dict(splits=[2, 3, 2]), dict(trees=[(0, 1), (2, 46)]),
               dict(trees=[(0, 1), (-1, 3)]), dict(trees=[(0, 1)]), dict(trees=[(0, 1), (2,)]), dict(breaks=breaks[:, :, :-1]),
               dict(breaks=breaks[:-1]), dict(count=count[:, :1]), dict(count=count[:, :, :-1]), dict(coef=coef[:, :-1]),
               dict(coef=coef[:1]), dict(coef=np.where(np.arange(9) == 2, np.nan, coef)), dict(coef=np.where(np.arange(9) == 2, np.inf, coef)),
               dict(w_out=0), dict(n_extra=1), dict(trees_per_pass=-1), dict(trees_per_pass=33), dict(s=3), dict(s=-1)):
        with pytest.raises(ValueError):
            e.tree_weights(**{**good, **kw})
    with pytest.raises(RuntimeError):
        e.tree_weights(**{**good, "s": 1})                           # split not set
    e.sync()

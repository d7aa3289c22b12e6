"""The tree-sort kernel (``csrc/k_qtree.hip``, ``Engine.tree_sorted_portfolios``) on a real MI355X
against the numpy path of ``analysis.tree_sorts`` (``tree_sort_numpy``, the definition), on the keys
the engine holds (bf16-rounded characteristics for a bf16 panel), and against the single- and
double-sort kernels.

Panel A (12 x 150 x 46): masked stocks, an empty period (5), a period of 7 stocks (2: fewer rows
than leaves, so nodes without rows at every shape), a constant column (0: every row in child 0, the other subtrees empty, their
breakpoints NaN), a column of 4 distinct values (1) and a column with both signed zeros (2). Panel B
(3 x 2600 x 5): three assign chunks, one extra key that only the lowest radix level separates
(1 + k 2^-23) and one of random fp32 values of both signs; its trees mix bf16 characteristics and
fp32 extra keys in every order (different key widths per level). Panel W (4 x 64 x 130): the wide
layer-0 path.

Counts and breakpoints are exact. A node's fp64 sum differs from numpy's float64 sum over the same
rows only by the summation order: both are within (m - 1) 2^-53 sum|v| of the exact sum for a node of
m <= n rows, so their difference is within n 2^-52 sum|v|, plus one ulp of the result (the bound of
the double-sort test, per node). It holds for the internal nodes too: a leaves-up sum is one more
ordering of the same m additions, and adding an empty child's zero is exact. Largest deviation
seen: profiles/tree_sorts_accuracy.txt."""
import itertools

import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_sorts as ts
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

KEYS_A = [0, 3, 1, 2, 4, 7, 45]
KEYS_B = [1, 5, 6, 2]                  # 5, 6: the extra keys
SPLITS = [(2, 2, 2), (2, 2, 2, 2, 2), (3, 3, 4), (2, 3, 2, 3), (16, 2), (2, 16), (6, 6)]


def _trees(keys, D, count):
    """``count`` trees of depth D on ``keys``: the rotations (every key at every level), then a
    repeated key, then mixed ones."""
    n = len(keys)
    out = [tuple(keys[(s + k) % n] for k in range(D)) for s in range(n)]
    out += [(keys[1],) * D, tuple(keys[(2 * k) % n] for k in range(D)), tuple(keys[-1 - k % 2] for k in range(D))]
    return out[:count]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


_PANELS = {}


def _panel(name):
    """batch, extra keys [E][T][N] (or None), extra values [K][T][N] (fp32 numpy)."""
    if name in _PANELS:
        return _PANELS[name]
    rng = np.random.default_rng(11)
    if name == "A":
        ret, feats, mask, mac = generate_panel_fast(12, 150, 46, 8, seed=0)
        assert bool(mask.all())
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False      # masked stocks
        mask[5] = False                                  # an empty period
        keep = torch.nonzero(mask[2]).flatten()[::19][:7]
        mask[2] = False
        mask[2, keep] = True                             # n = 7
        assert int(mask[2].sum()) == 7
        feats = feats.clone()
        feats[:, :, 0] = 0.375                           # constant
        feats[:, :, 1] = torch.bucketize(feats[:, :, 1].contiguous(), torch.tensor([-0.5, 0.0, 0.5])).float() - 1.5   # 4 values
        z = torch.arange(150) % 5
        feats[:, z == 0, 2] = -0.0
        feats[:, z == 1, 2] = 0.0
        extra = None
    elif name == "B":
        ret, feats, mask, mac = generate_panel_fast(3, 2600, 5, 8, seed=1)
        assert bool(mask.all())
        perm = np.stack([rng.permutation(2600) for _ in range(3)])
        low = (1.0 + perm.astype(np.float64) * 2.0 ** -23).astype(np.float32)
        assert all(len(np.unique(low[t])) == 2600 for t in range(3))
        both = (rng.standard_normal((3, 2600)) * 10.0 ** rng.integers(-3, 4, (3, 2600))).astype(np.float32)
        assert all(len(np.unique(both[t])) == 2600 for t in range(3))
        extra = np.stack([low, both])
    else:                                                # wide layer-0 path: F + Dm > 128
        ret, feats, mask, mac = generate_panel_fast(4, 64, 130, 8, seed=2)
        mask = mask.clone()
        mask[1, ::3] = False
        extra = None
    T, N = mask.shape
    # extra values over 12 decades, so that the fp64 node sums do round
    vals = (rng.standard_normal((2, T, N)) * 10.0 ** rng.integers(-6, 7, (2, T, N))).astype(np.float32)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    _PANELS[name] = (b, extra, vals)
    return _PANELS[name]


def _spec(F):
    return AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).spec


_ENGINES = {}


def _engine(name, precision, G=1):
    """One engine per (panel, precision, model count), with the panel's extra arrays on the device."""
    key = (name, precision, G)
    if key not in _ENGINES:
        from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
        b, extra, vals = _panel(name)
        eng = GANEngine(_spec(b["individual_features"].shape[2]), G, max_epochs=4, precision=precision)
        eng.set_data(b)
        if name == "W":
            assert int(eng.desc["wide"]) == 1
        ek = torch.as_tensor(extra).cuda().contiguous() if extra is not None else None
        vv = torch.as_tensor(vals).cuda().contiguous()
        torch.cuda.synchronize()
        _ENGINES[key] = (eng, ek, vv)
    return _ENGINES[key]


def _run(name, precision, trees, splits, G=1, n_values=0):
    eng, ek, vv = _engine(name, precision, G)
    out = eng.eng.tree_sorted_portfolios(0, [list(tr) for tr in trees], list(splits), ek.data_ptr() if ek is not None else 0,
                                         0 if ek is None else ek.shape[0], vv.data_ptr() if n_values else 0, n_values)
    eng.eng.sync()
    return out


_REFS = {}


def _ref(name, precision, trees, splits, n_values=0):
    """The numpy path on the keys the engine holds, and the same with |values| (for the bound)."""
    key = (name, precision, tuple(trees), tuple(splits), n_values)
    if key not in _REFS:
        b, extra, vals = _panel(name)
        f = b["individual_features"]
        keys = (_bf16_round(f) if precision == "bf16" else f).numpy().astype(np.float32)
        if extra is not None:
            keys = np.concatenate([keys, np.moveaxis(extra, 0, 2)], axis=2)
        v = np.concatenate([b["returns"].numpy().astype(np.float32)[:, :, None],
                            np.moveaxis(vals[:n_values], 0, 2)], axis=2)
        m = b["mask"].numpy()
        _REFS[key] = (ts.tree_sort_numpy(keys, trees, m, v, splits), ts.tree_sort_numpy(keys, trees, m, np.abs(v), splits)["sum"])
    return _REFS[key]


def _bits_equal(g, r):
    """bit for bit where finite (the sign of a zero included), NaN where the reference has NaN"""
    r = np.ascontiguousarray(np.asarray(r).astype(np.float32))
    g = np.ascontiguousarray(np.asarray(g))
    assert g.dtype == np.float32 and g.shape == r.shape
    assert (np.isnan(g) == np.isnan(r)).all()
    np.testing.assert_array_equal(np.where(np.isnan(r), 0, g.view(np.uint32)), np.where(np.isnan(r), 0, r.view(np.uint32)))


def _check_structure(got, splits, mask):
    """Children add up to their parent: the counts, and the sums in the fixed ascending order, bit
    for bit; the root holds the period's rows."""
    lay = ts.tree_layout(splits)
    off = lay["level_offsets"]
    cnt, sm = np.asarray(got["count"]), np.asarray(got["sum"])
    assert list(got["level_offsets"]) == off and list(got["break_offsets"]) == lay["break_offsets"]
    assert (cnt[:, :, 0] == mask.sum(1)[:, None]).all()
    for l in range(lay["depth"]):
        Q = splits[l]
        ch = cnt[:, :, off[l + 1]:off[l + 2]].reshape(cnt.shape[0], cnt.shape[1], -1, Q)
        np.testing.assert_array_equal(ch.sum(-1), cnt[:, :, off[l]:off[l + 1]])
        cs = sm[:, :, off[l + 1]:off[l + 2]].reshape(sm.shape[0], sm.shape[1], -1, Q, sm.shape[-1])
        x = cs[:, :, :, 0].copy()
        for q in range(1, Q):
            x = x + cs[:, :, :, q]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(sm[:, :, off[l]:off[l + 1]]).tobytes()


def _check(got, ref, absum, mask, splits):
    """Exact counts and breakpoints, sums within the fp64 accumulation bound; returns the largest
    deviation as a share of the bound."""
    cnt, sm, br = np.asarray(got["count"]), np.asarray(got["sum"]), np.asarray(got["breaks"])
    assert cnt.dtype == np.int32 and sm.dtype == np.float64 and br.dtype == np.float32
    assert cnt.shape == ref["count"].shape and sm.shape == ref["sum"].shape
    np.testing.assert_array_equal(cnt, ref["count"])
    _bits_equal(br, ref["breaks"])
    assert int(got["rows"]) == int(mask.sum())
    _check_structure(got, splits, mask)
    nt = mask.sum(1).astype(np.float64)
    bound = nt[:, None, None, None] * 2.0 ** -52 * absum + np.spacing(np.abs(ref["sum"]))
    dev = np.abs(sm - ref["sum"])
    worst = float((dev / bound).max()) if dev.size else 0.0
    print(f"largest |sum - numpy| / bound = {worst:.3f}, largest |sum - numpy| = {dev.max() if dev.size else 0.0:.3e}")
    assert (dev <= bound).all()
    return worst


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_a_matches_numpy(precision, splits):
    mask = _panel("A")[0]["mask"].numpy()
    trees = _trees(KEYS_A, len(splits), 8)
    got = _run("A", precision, trees, splits)
    ref, absum = _ref("A", precision, trees, splits)
    _check(got, ref, absum, mask, splits)
    cnt, br = np.asarray(got["count"]), np.asarray(got["breaks"])
    assert (cnt[5] == 0).all() and np.isnan(br[5]).all() and (np.asarray(got["sum"])[5] == 0).all()
    # the constant first key (tree 0): every row in child 0 of level 1, the other subtrees empty
    lay = ts.tree_layout(splits)
    off, boff = lay["level_offsets"], lay["break_offsets"]
    assert trees[0][0] == 0
    assert (cnt[:, 0, off[1]] == mask.sum(1)).all() and (cnt[:, 0, off[1] + 1:off[2]] == 0).all()
    if len(splits) > 1:
        live = [t for t in range(12) if t != 5]
        b2 = br[live][:, 0, boff[1]:boff[2]].reshape(len(live), splits[0], splits[1] - 1)
        assert np.isnan(b2[:, 1:]).all() and np.isfinite(b2[:, 0]).all()
    # period 2, n = 7: fewer rows than leaves, so every tree has empty leaves (and NaN breakpoints above them)
    assert (cnt[2, :, off[-2]:].sum(-1) == 7).all() and ((cnt[2, :, off[-2]:] == 0).sum(-1) >= lay["leaves"] - 7).all()
    assert float(got["gpu_ms"]) > 0


@pytest.mark.parametrize("splits", SPLITS + [(2, 2, 2, 2), (5, 5)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_b_long_periods_mixed_widths_and_values(precision, splits):
    mask = _panel("B")[0]["mask"].numpy()
    D = len(splits)
    # the tie-free extra key on every level, the rotations, then bf16 and fp32 keys in every order
    trees = list(dict.fromkeys([(5,) * D] + _trees(KEYS_B, D, 6) + list(itertools.product((1, 5), repeat=D))[:8]
                               + list(itertools.product((6, 2), repeat=D))[:4]))
    got = _run("B", precision, trees, splits, n_values=2)
    ref, absum = _ref("B", precision, trees, splits, n_values=2)
    _check(got, ref, absum, mask, splits)
    lay = ts.tree_layout(splits)
    assert np.asarray(got["sum"]).shape == (3, len(trees), lay["nodes"], 3)
    if splits == (2, 2, 2, 2):
        # tie-free keys (5 on every level): 2600 = 16 x 162.5, every leaf 162 or 163 rows
        p = trees.index((5, 5, 5, 5))
        leaves = np.asarray(got["count"])[:, p, lay["level_offsets"][4]:]
        assert ((leaves == 162) | (leaves == 163)).all()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_depth_1_equals_the_single_sort_kernel(precision):
    eng = _engine("A", precision)[0]
    for Q in (5, 16):
        got = _run("A", precision, [(c,) for c in KEYS_A], (Q,))
        one = eng.eng.sorted_portfolios(0, Q, KEYS_A)
        assert np.ascontiguousarray(np.asarray(got["count"])[:, :, 1:]).tobytes() == np.asarray(one["count"]).tobytes()
        assert np.asarray(got["breaks"]).tobytes() == np.asarray(one["breaks"]).tobytes()
    eng.eng.sync()


@pytest.mark.parametrize("n_values", [0, 1, 2])
@pytest.mark.parametrize("name,precision", [("A", "bf16"), ("A", "fp32"), ("B", "bf16"), ("B", "fp32")])
def test_depth_2_equals_the_double_sort_kernel(name, precision, n_values):
    eng, ek, vv = _engine(name, precision)
    pairs = [(0, 3), (1, 2), (3, 1), (4, 4), (7, 45)] if name == "A" else [(1, 5), (5, 2), (6, 3), (5, 6), (6, 5), (6, 6)]
    for Q in ((5, 5), (3, 12)):
        got = _run(name, precision, pairs, Q, n_values=n_values)
        two = eng.eng.double_sorted_portfolios(0, pairs, Q[0], Q[1], True, ek.data_ptr() if ek is not None else 0,
                                               0 if ek is None else ek.shape[0], vv.data_ptr() if n_values else 0, n_values)
        eng.eng.sync()
        lay = ts.tree_layout(Q)
        off, boff = lay["level_offsets"], lay["break_offsets"]
        cnt, sm, br = np.asarray(got["count"]), np.asarray(got["sum"]), np.asarray(got["breaks"])
        assert np.ascontiguousarray(cnt[:, :, off[2]:]).tobytes() == np.asarray(two["count"]).tobytes()
        assert np.ascontiguousarray(sm[:, :, off[2]:]).tobytes() == np.asarray(two["sum"]).tobytes()
        assert np.ascontiguousarray(br[:, :, :boff[1]]).tobytes() == np.asarray(two["breaks_a"]).tobytes()
        assert np.ascontiguousarray(br[:, :, boff[1]:]).tobytes() == np.asarray(two["breaks_b"]).tobytes()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_prefix_levels_equal_the_shorter_tree(precision):
    trees3 = _trees(KEYS_B, 3, 7)
    full = _run("B", precision, trees3, (2, 3, 4))
    short = _run("B", precision, [tr[:2] for tr in trees3], (2, 3))
    lay = ts.tree_layout((2, 3))
    nn, nb = lay["nodes"], lay["breaks"]
    assert np.ascontiguousarray(np.asarray(full["count"])[:, :, :nn]).tobytes() == np.asarray(short["count"]).tobytes()
    assert np.ascontiguousarray(np.asarray(full["breaks"])[:, :, :nb]).tobytes() == np.asarray(short["breaks"]).tobytes()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_repeatable_and_independent_of_the_models(precision):
    splits = (2, 3, 3)
    trees = _trees(KEYS_A, 3, 8)
    a = _run("A", precision, trees, splits, n_values=2)
    b2 = _run("A", precision, trees, splits, n_values=2)
    c = _run("A", precision, trees, splits, G=3, n_values=2)
    for k in ("count", "sum", "breaks"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b2[k]).tobytes()
        assert np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes()
    ref, absum = _ref("A", precision, trees, splits, n_values=2)
    _check(a, ref, absum, _panel("A")[0]["mask"].numpy(), splits)
    sel = [4, 0, 6, 2]
    sub = _run("A", precision, [trees[i] for i in sel], splits, n_values=2)
    for k in ("count", "sum", "breaks"):
        assert np.asarray(sub[k]).tobytes() == np.ascontiguousarray(np.asarray(a[k])[:, sel]).tobytes()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_path_engine(precision):
    mask = _panel("W")[0]["mask"].numpy()
    trees = [(0, 129, 64), (128, 64, 0), (77, 77, 77), (129, 1, 128)]
    for splits in ((2, 2, 2), (3, 3, 4)):
        got = _run("W", precision, trees, splits, n_values=1)
        ref, absum = _ref("W", precision, trees, splits, n_values=1)
        _check(got, ref, absum, mask, splits)
    assert np.asarray(got["count"]).shape == (4, 4, 49)


def test_bad_arguments():
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    b, _, vals = _panel("A")
    eng = GANEngine(_spec(46), 1, max_epochs=4)
    eng.set_data(b)
    vv = torch.zeros(3, 12, 150, device="cuda")
    torch.cuda.synchronize()
    e = eng.eng
    for kw in (dict(splits=[1, 2]), dict(splits=[2, 1]), dict(splits=[17, 2]), dict(splits=[2, 17]), dict(splits=[6, 7]),
               dict(splits=[4, 10]), dict(splits=[37], trees=[(0,)]), dict(splits=[2, 2, 2, 2, 3], trees=[(0,) * 5]),
               dict(splits=[2] * 6, trees=[(0,) * 6]), dict(splits=[], trees=[()]), dict(splits=[]),
               dict(trees=[(0, 1, 2)]), dict(trees=[(0,)]), dict(trees=[(0, 1), (0, 1, 2)]),
               dict(trees=[(46, 0)]), dict(trees=[(0, 46)]), dict(trees=[(-1, 0)]), dict(trees=[(0, -1)]),
               dict(trees=[(0, 47)], extra_keys=vv.data_ptr(), n_extra=1),
               dict(values=vv.data_ptr(), n_values=3), dict(n_values=-1), dict(n_values=1), dict(n_extra=1), dict(s=3), dict(s=-1)):
        with pytest.raises(ValueError):
            e.tree_sorted_portfolios(**{"s": 0, "trees": [(0, 1)], "splits": [2, 2], **kw})
    with pytest.raises(RuntimeError):
        e.tree_sorted_portfolios(1, [(0, 1)], [2, 2])          # split not set
    ok = e.tree_sorted_portfolios(0, [(45, 0, 45)], [2, 2, 2])
    assert np.asarray(ok["count"]).shape == (12, 1, 15) and np.asarray(ok["breaks"]).shape == (12, 1, 7)
    ok = e.tree_sorted_portfolios(0, [(46, 0, 46, 1, 46)], [2] * 5, extra_keys=vv.data_ptr(), n_extra=1)
    assert np.asarray(ok["count"]).shape == (12, 1, 63) and list(ok["level_offsets"]) == [0, 1, 3, 7, 15, 31, 63]
    assert list(ok["break_offsets"]) == [0, 1, 3, 7, 15, 31]
    ok = e.tree_sorted_portfolios(0, [(3, 4)], [6, 6], values=vv.data_ptr(), n_values=2)
    assert np.asarray(ok["sum"]).shape == (12, 1, 43, 3)
    e.sync()


def test_an_empty_tree_list():
    e = _engine("A", "bf16")[0].eng
    none = e.tree_sorted_portfolios(0, [], [2, 3, 3], n_values=0)
    assert np.asarray(none["count"]).shape == (12, 0, 27) and np.asarray(none["sum"]).shape == (12, 0, 27, 1)
    assert np.asarray(none["breaks"]).shape == (12, 0, 17) and float(none["gpu_ms"]) == 0.0
    assert list(none["level_offsets"]) == [0, 1, 3, 9, 27] and list(none["break_offsets"]) == [0, 1, 5, 17]
    assert int(none["rows"]) == int(_panel("A")[0]["mask"].sum())
    e.sync()


def test_python_api_cuda_matches_cpu():
    """One ensemble weight handed to both devices (evaluated by the engine): counts and breakpoints
    are equal once the CPU path sorts the bf16-rounded characteristics, and the priced results agree
    to 1e-9."""
    b = _panel("A")[0]
    models = []
    cfg = default_cli_config(8, 46, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)
    for g in range(2):
        torch.manual_seed(100 + g)
        models.append(AssetPricingGAN(cfg).eval())
    w = sp._gpu_weights(models, b).cpu().numpy()
    br = dict(b)
    br["individual_features"] = _bf16_round(b["individual_features"])
    trees = [(3, 4, 9), ("weight", 7, 7), (9, 46, 1), (1, 2, "weight"), (46, 46, 46)]
    r, m = b["returns"].numpy(), b["mask"].numpy()
    for splits in (None, (2, 3, 3)):
        gpu = ts.tree_sorted_portfolios(models, b, trees, splits=splits, device="cuda", weights=w)
        cpu = ts.tree_sorted_portfolios(models, br, trees, splits=splits, device="cpu", weights=w)
        assert gpu["names"] == cpu["names"] and gpu["names"][1] == "weight > x7 > x7"
        assert gpu["trees"] == cpu["trees"] and gpu["splits"] == cpu["splits"] and "gpu_ms" in gpu and "gpu_ms" not in cpu
        assert gpu["level_offsets"] == cpu["level_offsets"] and gpu["break_offsets"] == cpu["break_offsets"]
        np.testing.assert_array_equal(gpu["count"], cpu["count"])
        np.testing.assert_array_equal(gpu["breaks"], cpu["breaks"])
        pg, pc = ts.price_tree_sorted(gpu, w, r, m), ts.price_tree_sorted(cpu, w, r, m)
        for k in ("mean_ret", "alpha", "t_alpha", "ev_asset", "tree_ev", "tree_xs_r2", "tree_mean_abs_alpha", "hml",
                  "hml_sharpe", "ev", "xs_r2", "mean_abs_alpha", "leaves_ev", "leaves_xs_r2", "leaves_mean_abs_alpha"):
            np.testing.assert_allclose(np.asarray(pg[k]), np.asarray(pc[k]), rtol=1e-9, atol=0, equal_nan=True, err_msg=k)
        assert pg["assets"] == pc["assets"] and pg["leaves"] == pc["leaves"]
    f32 = ts.tree_sorted_portfolios(models, b, trees, device="cuda", weights=w, precision="fp32")
    ex = ts.tree_sorted_portfolios(models, b, trees, device="cpu", weights=w)
    np.testing.assert_array_equal(f32["count"], ex["count"])


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    """``tree_sorts`` on both devices: the same report layout and assets, the rest of the result
    unchanged. (The numbers differ by the towers' precision and by the rows the bf16 panel moves
    across a breakpoint, so only the structure is compared.)"""
    import os
    import golden_cases as gc
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    capsys.readouterr()
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=True, tree_sorts="0:1:2,weight:3:3")
    tg = capsys.readouterr().out
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", verbose=True, tree_sorts="0:1:2,weight:3:3")
    tc = capsys.readouterr().out
    head = "TREE-SORTED PORTFOLIOS"
    print(tg[tg.index(head):])
    print(tc[tc.index(head):])
    assert set(gpu) == set(plain) | {"tree_sorts"}
    for k in plain:
        assert gpu[k] == plain[k]
    g, c = gpu["tree_sorts"], cpu["tree_sorts"]
    assert "gpu_ms" in g["portfolios"] and "gpu_ms" not in c["portfolios"]
    assert g["portfolios"]["names"] == c["portfolios"]["names"] and len(g["portfolios"]["names"]) == 2
    assert g["portfolios"]["trees"] == c["portfolios"]["trees"] == [(0, 1, 2), (46, 3, 3)]
    assert g["portfolios"]["count"].shape == c["portfolios"]["count"].shape == (60, 2, 15)
    np.testing.assert_array_equal(g["portfolios"]["count"][:, :, 0], c["portfolios"]["count"][:, :, 0])
    assert set(g["priced"]) == set(c["priced"])
    assert g["priced"]["assets"] == c["priced"]["assets"] == 29 and g["priced"]["leaves"] == 16
    assert np.isfinite(g["priced"]["hml"]).all() and np.isfinite(g["priced"]["ev"]) and np.isfinite(g["priced"]["tree_ev"]).all()
    assert len(tg[tg.index(head):].splitlines()) == len(tc[tc.index(head):].splitlines())

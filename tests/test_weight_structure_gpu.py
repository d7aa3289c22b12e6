"""The weight-structure kernel (``csrc/k_wsurf.hip``, ``Engine.weight_surface``) on a real MI355X.

Reference op: `SDFNetwork.forward` in evaluation mode on generated rows. Two references are used:
the engine's own evaluation forward (``forward_split``) on a second engine whose panel holds the
generated rows as its stocks in every period (bitwise, and the fp64 sum of ``s * w``), and the
float64 CPU path of ``analysis.weight_structure``. The panel is the one of
``tests/test_importance_gpu.py``: masked stocks and an empty period 5.

Item sets (rows are 32 to a tile; at these sizes a workgroup's eight waves share one tile's periods,
``test_every_chunking_gives_the_same_bits`` reaches the launch's other chunkings):
  small  P = 5, curves 0 / 7 / 45, surfaces (0,45) (8,31) (32,7): 90 rows, two full tiles and a
         26-row tail, tiles spanning items; columns on a lane-group edge, a k-step edge, the last one;
  large  P = 9, all F curves and 12 surfaces, one with its columns descending: 1386 rows, 43 full
         tiles and a 10-row tail, 44 workgroups;
  F = 20 the same pattern with columns 0, 7, 8 and 19."""
import copy
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.analysis import weight_structure as wst
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

T_ = 12
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _batch(F=46):
    if F not in _PANELS:
        ret, feats, mask, mac = generate_panel_fast(T_, 150, F, 8, seed=0)
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False  # masked stocks
        mask[5] = False                              # an empty period
        _PANELS[F] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[F]


ARCHS = {
    "h64x2_r4": (46, dict(hidden_dim=[64, 64], rnn_dim=[4])),
    "h64_r8": (46, dict(hidden_dim=[64], rnn_dim=[8])),
    "h48_32_r2x2": (46, dict(hidden_dim=[48, 32], rnn_dim=[2, 2])),
    "h64x4_r4": (46, dict(hidden_dim=[64] * 4, rnn_dim=[4])),
    "no_rnn": (46, dict(hidden_dim=[64, 64], use_lstm=False)),
    "F20": (20, dict(hidden_dim=[64, 64], rnn_dim=[4])),
}


def _models(name, G=1):
    F, kw = ARCHS[name]
    cfg = default_cli_config(8, F, dropout=0.05, **kw)
    out = []
    for g in range(G):
        torch.manual_seed(100 + g)
        out.append(AssetPricingGAN(cfg).eval())
    return out


def _sets(F):
    """name -> (grid, base, items): float32 grid and base, curves first."""
    rng = np.random.default_rng(7)
    base = (rng.standard_normal(F) * 0.2).astype(np.float32)
    g5 = np.linspace(-0.45, 0.45, 5).astype(np.float32)
    g9 = np.linspace(-0.6, 0.5, 9).astype(np.float32)
    if F == 46:
        small = [(0, -1), (7, -1), (45, -1), (0, 45), (8, 31), (32, 7)]
        pairs = [(45, 0), (0, 1), (7, 8), (31, 32), (8, 31), (32, 7), (15, 16), (16, 40), (44, 45), (3, 29), (23, 24), (1, 33)]
    else:
        small = [(0, -1), (7, -1), (19, -1), (0, 19), (8, 7), (19, 8)]
        pairs = [(19, 0), (0, 1), (7, 8), (8, 19), (0, 7), (8, 7), (15, 16), (16, 3), (18, 19), (3, 12), (11, 12), (1, 17)]
    large = [(a, -1) for a in range(F)] + pairs
    return {"small": (g5, base, small), "large": (g9, base, large)}


def _nrows(grid, items):
    P = len(grid)
    return sum(P if b < 0 else P * P for _, b in items)


def _rows(grid, base, items):
    cols = [a for a, b in items if b < 0]
    prs = [(a, b) for a, b in items if b >= 0]
    return wst.make_rows(grid.astype(np.float64), base.astype(np.float64), cols, prs).astype(np.float32)


def _engine(models, b, precision):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    eng = GANEngine(models[0].spec, len(models), max_epochs=4, precision=precision)
    eng.set_data(b)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    return eng


def _surface(models, b, precision, grid, base, items, scale=None, calls=1, full=False):
    """values of Engine.weight_surface; scale: [G, T] or ones."""
    eng = _engine(models, b, precision)
    ptr, keep = 0, None
    if scale is not None:
        keep = torch.as_tensor(np.asarray(scale, dtype=np.float32)).cuda().contiguous()
        assert tuple(keep.shape) == (len(models), b["mask"].shape[0])
        torch.cuda.synchronize()
        ptr = keep.data_ptr()
    res = [eng.eng.weight_surface(0, ptr, [float(x) for x in grid], [float(x) for x in base], items)
           for _ in range(calls)]
    eng.eng.sync()
    for r in res:
        assert r["rows"] == _nrows(grid, items) == len(r["values"])
    if not full:
        res = [np.asarray(r["values"]) for r in res]
    return res[0] if calls == 1 else res


_REFW = {}


def _ref_w(name, precision, setname, G=1):
    """Raw weights [G, T, rows] (float32) of forward_split on an engine whose panel has the set's
    generated rows as its stocks in every period (same macro series, same models)."""
    key = (name, precision, setname, G)
    if key not in _REFW:
        F = ARCHS[name][0]
        grid, base, items = _sets(F)[setname]
        rows = _rows(grid, base, items)
        R = rows.shape[0]
        b = _batch(F)
        fake = {"returns": torch.zeros(T_, R), "individual_features": torch.as_tensor(rows)[None].repeat(T_, 1, 1),
                "mask": torch.ones(T_, R, dtype=torch.bool), "macro_features": b["macro_features"]}
        eng = _engine(_models(name, G), fake, precision)
        eng.eng.forward_split(0, False, False)
        w = np.stack([np.asarray(eng.eng.read_ws(g, 0, "w"))[:T_ * R].reshape(T_, R) for g in range(G)])
        eng.eng.sync()
        _REFW[key] = w
        _REFW[key].setflags(write=False)
    return _REFW[key]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ARCHS))
def test_bitwise_against_the_forward(name, precision):
    F = ARCHS[name][0]
    m, b = _models(name), _batch(F)
    for setname, (grid, base, items) in _sets(F).items():
        assert _nrows(grid, items) == {"small": 90, "large": 9 * F + 12 * 81}[setname]
        ref = _ref_w(name, precision, setname)
        for t in (3, 5):                              # a normal period and the empty one
            sc = np.zeros((1, T_), dtype=np.float32)
            sc[0, t] = 1.0
            got = _surface(m, b, precision, grid, base, items, scale=sc)
            np.testing.assert_array_equal(got, ref[0, t], err_msg=f"{setname} period {t}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_bitwise_sum_over_many_periods(precision):
    """70 periods, two models, scales that are powers of two (or zero): s * w is exact, so the
    kernel's fma sequence is the float32 sum of the forward's weights in (g, t) order, bit for bit.
    The waves that share a tile exchange 32 periods per round here: two full rounds and a partial."""
    T, G = 70, 2
    grid, base, items = _sets(46)["small"]
    rows = _rows(grid, base, items)
    R = rows.shape[0]
    ret, feats, mask, mac = generate_panel_fast(T, 40, 46, 8, seed=1)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    fake = {"returns": torch.zeros(T, R), "individual_features": torch.as_tensor(rows)[None].repeat(T, 1, 1),
            "mask": torch.ones(T, R, dtype=torch.bool), "macro_features": mac}
    models = _models("h64x2_r4", G)
    eng = _engine(models, fake, precision)
    eng.eng.forward_split(0, False, False)
    w = np.stack([np.asarray(eng.eng.read_ws(g, 0, "w"))[:T * R].reshape(T, R) for g in range(G)])
    eng.eng.sync()
    del eng
    rng = np.random.default_rng(13)
    sc = (2.0 ** rng.integers(-3, 2, size=(G, T))).astype(np.float32)
    sc[rng.random((G, T)) < 0.15] = 0.0
    ref = np.zeros(R, dtype=np.float32)
    for g in range(G):
        for t in range(T):
            if sc[g, t] != 0:
                ref = (ref + sc[g, t] * w[g, t]).astype(np.float32)
    got = _surface(models, b, precision, grid, base, items, scale=sc, full=True)
    assert got["period_split"] == 8
    np.testing.assert_array_equal(np.asarray(got["values"]), ref)


def _bound(s, w):
    """Sequential fp32 summation bound per cell: (G T + 1) 2^-24 sum |s w|, and the fp64 sum."""
    sw = np.asarray(s, dtype=np.float64)[:, :, None] * w.astype(np.float64)
    return (sw.shape[0] * sw.shape[1] + 1) * EPS * np.abs(sw).sum((0, 1)), sw.sum((0, 1))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_summation(precision):
    name, G = "h64x2_r4", 3
    grid, base, items = _sets(46)["large"]
    w = _ref_w(name, precision, "large", G)
    sc = (np.random.default_rng(3).random((G, T_)) * 0.2 + 0.01).astype(np.float32)
    got = _surface(_models(name, G), _batch(), precision, grid, base, items, scale=sc)
    bound, ref = _bound(sc, w)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"summation {precision}: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def _values(r):
    return np.concatenate([np.asarray(r["curves"]).ravel(), np.asarray(r["surfaces"]).ravel()])


def _structure_kw(F, setname):
    grid, base, items = _sets(F)[setname]
    return dict(grid=grid, base=base, characteristics=[a for a, b in items if b < 0],
                pairs=[(a, b) for a, b in items if b >= 0])


_REF64 = {}


def _ref64(name, scale):
    key = (name, scale)
    if key not in _REF64:
        F = ARCHS[name][0]
        _REF64[key] = wst.weight_structure(_models(name), _batch(F), scale=scale, dtype=torch.float64,
                                           **_structure_kw(F, "large"))
    return _REF64[key]


def _maxrel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _cos(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("name", list(ARCHS))
def test_fp32_engine_matches_float64_cpu_path(name, capsys):
    F = ARCHS[name][0]
    ref = _ref64(name, "ensemble")
    got = wst.weight_structure(_models(name), _batch(F), device="cuda", precision="fp32", **_structure_kw(F, "large"))
    assert "using the CPU path" not in capsys.readouterr().out
    assert got["periods_used"].tolist() == ref["periods_used"].tolist() == [T_ - 1]
    err, eo = _maxrel(_values(got), _values(ref)), abs(got["offset"][0] - ref["offset"][0]) / np.abs(_values(ref)).max()
    print(f"fp32 {name}: values max-rel {err:.3e}  offset {eo:.3e}")
    rec = os.environ.get("DLAP_WSURF_RECORD")
    if rec:
        with open(rec, "a") as fh:
            fh.write(f"fp32 {name:12s} values max-rel {err:.3e}  offset {eo:.3e}\n")
    assert err <= 1e-5 and eo <= 1e-5, (err, eo)     # the project's fp32 acceptance bound


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _emulated(name):
    """ref64's computation with the grid, the base row and the tower's weight matrices (hidden
    layers and the output row: the kernel's operand fragments) rounded to bf16."""
    F = ARCHS[name][0]
    kw = _structure_kw(F, "large")
    kw["grid"] = _bf16_round(torch.as_tensor(kw["grid"])).numpy()
    kw["base"] = _bf16_round(torch.as_tensor(kw["base"])).numpy()
    m = copy.deepcopy(_models(name)[0])
    with torch.no_grad():
        for layer in list(m.sdf_net.fc_layers) + [m.sdf_net.output_proj]:
            if isinstance(layer, torch.nn.Linear):
                layer.weight.copy_(_bf16_round(layer.weight))
    return wst.weight_structure([m], _batch(F), scale="raw", dtype=torch.float64, **kw)


@pytest.mark.parametrize("name", list(ARCHS))
def test_bf16_engine_within_measured_bound(name, capsys):
    """relL2(kernel, ref64) <= 8 e_emu, e_emu the error of bf16-rounded grid, base and weight
    matrices alone: the kernel also rounds the per-period inputs and every layer's activations.
    Never above the project's bf16 bound (err < 0.08, cos > 0.998). scale="raw": the scale table is
    the same on both sides, so the comparison is of the towers on the generated rows only."""
    F = ARCHS[name][0]
    ref, emu = _values(_ref64(name, "raw")), _values(_emulated(name))
    got = _values(wst.weight_structure(_models(name), _batch(F), device="cuda", scale="raw", **_structure_kw(F, "large")))
    assert "using the CPU path" not in capsys.readouterr().out
    e_emu, err, cs = _rel_l2(emu, ref), _rel_l2(got, ref), _cos(got, ref)
    line = f"bf16 {name:12s} relL2 {err:.3e}  e_emu {e_emu:.3e}  ratio {err / e_emu:5.2f}  cos {cs:.6f}"
    print(line)
    rec = os.environ.get("DLAP_WSURF_RECORD")
    if rec:
        with open(rec, "a") as fh:
            fh.write(line + "\n")
    assert err <= 8 * e_emu, (err, e_emu)
    assert err < 0.08 and cs > 0.998, (err, cs)


def test_repeatable_and_batching_invariant():
    b, G = _batch(), 3
    models = _models("h64x2_r4", G)
    grid, base, items = _sets(46)["large"]
    sc = (np.random.default_rng(5).random((G, T_)) * 0.2 + 0.01).astype(np.float32)
    first, second = _surface(models, b, "bf16", grid, base, items, scale=sc, calls=2)
    np.testing.assert_array_equal(first, second)
    for g in range(G):
        only = np.zeros_like(sc)
        only[g] = sc[g]
        solo = _surface([models[g]], b, "bf16", grid, base, items, scale=sc[g:g + 1])
        np.testing.assert_array_equal(solo, _surface(models, b, "bf16", grid, base, items, scale=only))


def test_position_invariant():
    b = _batch()
    models = _models("h64x2_r4", 2)
    grid, base, items = _sets(46)["large"]
    whole = _surface(models, b, "bf16", grid, base, items)
    P, n1 = len(grid), 46
    for j in (0, 7, 45, 46, 46 + 5, 46 + 11):           # curves and surfaces, first / inner / last
        a, c = items[j]
        lo = j * P if c < 0 else n1 * P + (j - n1) * P * P
        alone = _surface(models, b, "bf16", grid, base, [items[j]])
        np.testing.assert_array_equal(alone, whole[lo:lo + len(alone)], err_msg=str(items[j]))


_ALONE = {}


@pytest.mark.parametrize("n2,split,tpw", [(64, 4, 1), (150, 2, 1), (330, 1, 1), (1035, 1, 2)])
def test_every_chunking_gives_the_same_bits(n2, split, tpw):
    """The launch picks its chunking from the number of tiles against the device's 1024 SIMDs: eight
    waves share a tile's periods below 256 tiles (every set above), four below 512, two below 1024,
    then a wave owns one tile, and two from 4096 tiles. All 46 curves and the first n2 pairs at
    P = 12 (552 + 144 n2 rows: 306 / 693 / 1503 / 4675 tiles) reach the other four paths; an item
    gets the bits it gets alone (the eight-wave path, checked against the forward above)."""
    b = _batch()
    models = _models("h64x2_r4", 2)
    grid = np.linspace(-0.5, 0.5, 12).astype(np.float32)
    base = _sets(46)["small"][1]
    sc = (np.random.default_rng(11).random((2, T_)) * 0.2 + 0.01).astype(np.float32)
    sc[:, 5] = 0.0
    items = [(a, -1) for a in range(46)] + [(a, c) for a in range(46) for c in range(a + 1, 46)][:n2]
    whole = _surface(models, b, "bf16", grid, base, items, scale=sc, full=True)
    assert (whole["period_split"], whole["tiles_per_wave"]) == (split, tpw)
    assert whole["rows"] == 46 * 12 + n2 * 144
    v = np.asarray(whole["values"])
    for j in (0, 45, 46, 46 + 37, 46 + 63):
        if j not in _ALONE:
            alone = _surface(models, b, "bf16", grid, base, [items[j]], scale=sc, full=True)
            assert (alone["period_split"], alone["tiles_per_wave"]) == (8, 1)
            _ALONE[j] = np.asarray(alone["values"])
        lo = j * 12 if j < 46 else 46 * 12 + (j - 46) * 144
        np.testing.assert_array_equal(_ALONE[j], v[lo:lo + len(_ALONE[j])], err_msg=str(items[j]))
    np.testing.assert_array_equal(_surface(models, b, "bf16", grid, base, items[-1:], scale=sc), v[-144:])


def test_groups_add_up():
    name, G = "h64x2_r4", 3
    grid, base, items = _sets(46)["large"]
    w = _ref_w(name, "bf16", "large", G)
    sc = (np.random.default_rng(9).random((G, T_)) * 0.2 + 0.01).astype(np.float32)
    grp = np.arange(T_) % 3 == 0
    s0, s1 = sc * grp[None], sc * ~grp[None]
    models, b = _models(name, G), _batch()
    v = [_surface(models, b, "bf16", grid, base, items, scale=s).astype(np.float64) for s in (s0, s1, sc)]
    bound, _ = _bound(sc, w)
    assert (np.abs(v[0] + v[1] - v[2]) <= bound).all()
    # and through the Python interface: periods_used-weighted group results equal the whole
    kw = dict(device="cuda", scale="raw", **_structure_kw(46, "small"))
    whole = wst.weight_structure(models, b, **kw)
    parts = wst.weight_structure(models, b, period_groups=np.where(grp, 0, 1), **kw)
    assert parts["periods_used"].tolist() == [4, 8] and whole["periods_used"].tolist() == [T_]
    tot = sum(parts["periods_used"][k] * _values({"curves": parts["curves"][k], "surfaces": parts["surfaces"][k]})
              for k in range(2)) / T_
    assert _maxrel(tot, _values(whole)) <= 1e-5


def test_engine_argument_errors():
    b = _batch()
    eng = _engine(_models("h64x2_r4"), b, "bf16")
    e = eng.eng
    g, x0 = [0.0, 1.0], [0.0] * 46
    for kw, msg in ((dict(grid=g, base=x0, items=[(1, 1)]), "different columns"),
                    (dict(grid=g, base=x0, items=[(1, 46)]), "outside"),
                    (dict(grid=g, base=x0, items=[(-1, -1)]), "outside"),
                    (dict(grid=[0.0], base=x0, items=[(0, -1)]), "2 .. 64"),
                    (dict(grid=[0.0] * 65, base=x0, items=[(0, -1)]), "2 .. 64"),
                    (dict(grid=g, base=x0[:-1], items=[(0, -1)]), "base"),
                    (dict(grid=g, base=x0, items=[]), "no items"),
                    (dict(grid=g, base=x0, items=[(0, 1), (2, -1)]), "curves go before")):
        with pytest.raises(ValueError, match="weight_surface.*" + msg):
            e.weight_surface(0, 0, **kw)
    with pytest.raises(ValueError, match="weight_surface: split not set"):
        e.weight_surface(1, 0, g, x0, [(0, -1)])
    assert e.weight_surface_supported(0) and not e.weight_surface_supported(1)
    e.sync()


def test_wide_shape_raises_and_falls_back(capsys):
    ret, feats, mask, mac = generate_panel_fast(T_, 150, 200, 8, seed=0)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    torch.manual_seed(100)
    m = AssetPricingGAN(default_cli_config(8, 200, dropout=0.05)).eval()
    eng = _engine([m], b, "bf16")
    assert not eng.eng.weight_surface_supported(0)
    with pytest.raises(ValueError, match="weight_surface"):
        eng.eng.weight_surface(0, 0, [0.0, 1.0], [0.0] * 200, [(0, -1)])
    eng.eng.sync()
    del eng
    kw = dict(grid=np.linspace(-0.4, 0.4, 5), characteristics=[0, 199], pairs=[(0, 199)])
    got = wst.weight_structure([m], b, device="cuda", **kw)
    assert "using the CPU path" in capsys.readouterr().out
    ref = wst.weight_structure([m], b, device="cpu", **kw)
    for k in ("curves", "surfaces", "offset", "interaction", "periods_used"):
        np.testing.assert_array_equal(got[k], ref[k])


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    kw = dict(weight_structure=True, structure_points=9, structure_pairs="0:45,8:31,32:7")
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False, **kw)
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", verbose=False, **kw)
    assert "using the CPU path" not in capsys.readouterr().out
    for k in plain:
        assert gpu[k] == plain[k], k
    a, c = gpu["weight_structure"], cpu["weight_structure"]
    assert a["names"] == c["names"] and a["pair_items"] == c["pair_items"] == [(0, 45), (8, 31), (32, 7)]
    assert a["periods_used"].tolist() == c["periods_used"].tolist() == [60]
    err, cs = _rel_l2(_values(a), _values(c)), _cos(_values(a), _values(c))
    print(f"end to end: relL2 {err:.3e} cos {cs:.6f} offset {a['offset'][0]:.4e} / {c['offset'][0]:.4e}")
    assert err < 0.08 and cs > 0.998, (err, cs)
    assert abs(a["offset"][0] - c["offset"][0]) < 0.08 * np.abs(_values(c)).max()

"""The input-gradient kernel (``csrc/k_sens.hip``, ``Engine.input_sensitivity``) on a real MI355X.

Reference op: torch autograd of `SDFNetwork.forward` in evaluation mode with respect to its
concatenated input -- here the CPU path of ``analysis.importance`` in float64 (``ref64``) on the
same models. The panel has masked stocks, an empty period and a row count that is no multiple of
the 32-row tile (R = 11 * 129 = 1419: six chunks of eight tiles, the last one partial)."""
import copy
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.analysis import importance as imp
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _batch(F=46):
    if F not in _PANELS:
        ret, feats, mask, mac = generate_panel_fast(12, 150, F, 8, seed=0)
        assert bool(mask.all())                      # the generator's panel is complete
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False  # masked stocks
        mask[5] = False                              # an empty period
        assert int(mask.sum()) == 11 * 129
        _PANELS[F] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[F]


# name -> (F, config keywords)
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


_REF = {}


def _ref64(name):
    """abs [1, C], sum [1, C], ens [C] of model 0 with scale one, CPU autograd in float64."""
    if name not in _REF:
        _REF[name] = imp._cpu_sums(_models(name), _batch(ARCHS[name][0]), "raw", torch.float64)
    return _REF[name]


def _engine(models, b, precision="bf16", scale=None, calls=1):
    """Raw sums of Engine.input_sensitivity for the models (one architecture); scale: [G, T] or ones."""
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    eng = GANEngine(models[0].spec, len(models), max_epochs=4, precision=precision)
    eng.set_data(b)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    ptr, keep = 0, None
    if scale is not None:
        keep = torch.as_tensor(np.asarray(scale, dtype=np.float32)).cuda().contiguous()
        assert tuple(keep.shape) == (len(models), b["mask"].shape[0])
        torch.cuda.synchronize()
        ptr = keep.data_ptr()
    res = [eng.eng.input_sensitivity(0, ptr) for _ in range(calls)]
    eng.eng.sync()
    return res[0] if calls == 1 else res


def _maxrel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _cos(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("name", list(ARCHS))
def test_fp32_engine_matches_float64_autograd(name):
    ref = _ref64(name)
    got = _engine(_models(name), _batch(ARCHS[name][0]), "fp32")
    assert got["rows"] == ref["rows"] == 1419
    for k in ("abs", "sum", "ens"):
        err = _maxrel(got[k], ref[k])
        print(f"fp32 {name} {k}: max-rel {err:.3e}")
        assert err <= 1e-5, (k, err)      # the project's fp32 acceptance bound


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _emulated(name):
    """ref64's computation with the panel and the tower's weight matrices rounded to bf16."""
    b = dict(_batch(ARCHS[name][0]))
    b["individual_features"] = _bf16_round(b["individual_features"])
    m = copy.deepcopy(_models(name)[0])
    with torch.no_grad():
        for layer in m.sdf_net.fc_layers:
            if isinstance(layer, torch.nn.Linear):
                layer.weight.copy_(_bf16_round(layer.weight))
    return imp._cpu_sums([m], b, "raw", torch.float64)


@pytest.mark.parametrize("name", list(ARCHS))
def test_bf16_engine_within_measured_bound(name):
    """relL2(kernel, ref64) <= 8 e_emu, e_emu the error of bf16-rounded inputs and weights alone:
    the kernel also rounds every layer's activations and every dz -- about three times as many
    rounding sites, adding at worst linearly; the rest of the factor is headroom. Never above the
    project's bf16-against-fp32 gradient bound (err < 0.08, cos > 0.998)."""
    ref, emu = _ref64(name), _emulated(name)
    got = _engine(_models(name), _batch(ARCHS[name][0]), "bf16")
    lines = []
    for k in ("abs", "sum", "ens"):
        e_emu, err, cs = _rel_l2(emu[k], ref[k]), _rel_l2(got[k], ref[k]), _cos(got[k], ref[k])
        lines.append(f"{name:12s} {k:3s} relL2 {err:.3e}  e_emu {e_emu:.3e}  ratio {err / e_emu:5.2f}  cos {cs:.6f}")
        print(lines[-1])
    rec = os.environ.get("DLAP_SENS_RECORD")
    if rec:
        with open(rec, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    for k in ("abs", "sum", "ens"):
        e_emu, err, cs = _rel_l2(emu[k], ref[k]), _rel_l2(got[k], ref[k]), _cos(got[k], ref[k])
        assert err <= 8 * e_emu, (k, err, e_emu)
        assert err < 0.08 and cs > 0.998, (k, err, cs)


def test_batched_members_equal_solo_and_calls_repeat():
    b = _batch()
    models = _models("h64x2_r4", G=3)
    first, second = _engine(models, b, calls=2)
    for k in ("abs", "sum", "ens"):
        np.testing.assert_array_equal(first[k], second[k])
    for g in range(3):
        solo = _engine([models[g]], b)
        np.testing.assert_array_equal(solo["abs"][0], first["abs"][g])
        np.testing.assert_array_equal(solo["sum"][0], first["sum"][g])


def test_ensemble_semantics():
    b = _batch()
    m = _models("h64x2_r4")[0]
    T = b["mask"].shape[0]
    solo = _engine([m], b)                                    # scale = ones, G = 1
    np.testing.assert_array_equal(solo["ens"], solo["abs"][0])
    opp = _engine([m, m], b, scale=np.stack([np.full(T, 0.5), np.full(T, -0.5)]))
    assert (opp["ens"] == 0).all()
    np.testing.assert_array_equal(opp["abs"][0], opp["abs"][1])
    np.testing.assert_array_equal(opp["sum"][0], -opp["sum"][1])
    same = _engine([m, m], b, scale=np.full((2, T), 0.5))
    assert _maxrel(same["ens"], solo["abs"][0]) <= 1e-5


@pytest.mark.parametrize("name", ["h64x2_r4", "no_rnn", "F20"])
def test_no_padding_columns(name):
    F = ARCHS[name][0]
    m = _models(name)[0]
    got = _engine([m], _batch(F))
    Dm = 8 if name == "no_rnn" else 4
    assert got["abs"].shape == (1, F + Dm) and got["sum"].shape == (1, F + Dm) and got["ens"].shape == (F + Dm,)
    for k in ("abs", "sum", "ens"):
        assert np.isfinite(got[k]).all()
    assert (got["abs"] > 0).all()


def test_wide_shape_raises_and_falls_back(capsys):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    ret, feats, mask, mac = generate_panel_fast(12, 150, 200, 8, seed=0)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    torch.manual_seed(100)
    m = AssetPricingGAN(default_cli_config(8, 200, dropout=0.05)).eval()
    eng = GANEngine(m.spec, 1, max_epochs=4)
    eng.set_data(b)
    eng.set_model(0, m, 0)
    with pytest.raises(ValueError, match="input_sensitivity"):
        eng.eng.input_sensitivity(0, 0)
    eng.eng.sync()
    del eng
    got = imp.variable_importance([m], b, device="cuda")
    assert "using the CPU path" in capsys.readouterr().out
    ref = imp.variable_importance([m], b, device="cpu")
    for k in ("abs_mean", "per_model_abs_mean", "per_model_signed_mean", "characteristics", "state"):
        np.testing.assert_array_equal(got[k], ref[k])


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False, importance=True)
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", verbose=False, importance=True)
    assert "using the CPU path" not in capsys.readouterr().out
    for k in plain:
        assert gpu[k] == plain[k], k
    a, c = gpu["variable_importance"], cpu["variable_importance"]
    assert a["names"] == c["names"] and a["rows"] == c["rows"]
    for k in ("abs_mean", "per_model_abs_mean", "characteristics", "state"):
        err, cs = _rel_l2(a[k], c[k]), _cos(a[k], c[k])
        print(f"end to end {k}: relL2 {err:.3e} cos {cs:.6f}")
        assert err < 0.08 and cs > 0.998, (k, err, cs)

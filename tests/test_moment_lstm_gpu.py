"""The moment network's own macro LSTM (config key ``moment_lstm``) on the native engine
(k_mlstm.hip) against the CPU trainer and torch's LSTM: training trajectories, the per-period
bias table the moment towers read, a split longer than any LDS-staged limit, the phase-2
gradients alone, determinism / batching invariance, the bf16 engine's gap, the phase plans and
the setup-time limits, and one short full schedule.

The harness (``_splits``, the trajectories, ``_tensor_errors``, ``TOL``, ``NOISE_ONLY``) is a copy of
tests/test_engine_fp32_gpu.py's."""
import copy
import os

import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

TOL = 1e-5
LSTM_KEYS = [f"moment_net.macro_lstm.lstm.{n}_l0" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


def _splits(T=(36, 12, 18), N=160, F=46, M=8, seed=0):
    ret, feats, mask, mac = generate_panel_fast(sum(T), N, F, M, seed=seed)
    mac = (mac - mac[:T[0]].mean(0)) / (mac[:T[0]].std(0, unbiased=False) + 1e-8)
    cuts = [(0, T[0]), (T[0], T[0] + T[1]), (T[0] + T[1], sum(T))]
    return [{"returns": ret[a:b].contiguous(), "individual_features": feats[a:b].contiguous(),
             "mask": mask[a:b].contiguous(), "macro_features": mac[a:b].contiguous()} for a, b in cuts]


def _cpu_trajectory(model, b, sched, lr):
    """Per-step (loss, grad norm) of the reference step function on ``model`` (modified in place)."""
    from deeplearninginassetpricing_paperreplication_amd.train.trainer import train_epoch
    opt_s = torch.optim.Adam(model.sdf_net.parameters(), lr=lr)
    opt_m = torch.optim.Adam(model.moment_net.parameters(), lr=lr)
    out = []
    for phase, n in sched:
        for _ in range(n):
            if phase == 2:                     # SDF frozen
                for p in model.sdf_net.parameters():
                    p.requires_grad_(False)
                r = train_epoch(model, opt_m, b, "cpu", "moment", scope="moment")
                for p in model.sdf_net.parameters():
                    p.requires_grad_(True)
            else:
                r = train_epoch(model, opt_s, b, "cpu", "unconditional" if phase == 1 else "conditional",
                                scope="sdf")
            out.append((r["loss"], r["grad_norm"]))
    return np.array(out, np.float64)


def _gpu_trajectory(model, splits, sched, lr, precision="fp32", use_graph=True, others=(), slot=0):
    """Train ``model`` at position ``slot`` of an engine that batches it with ``others``."""
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine, HIST
    members = list(others)
    members.insert(slot, model)
    eng = GANEngine(model.spec, len(members), max_epochs=64, precision=precision)
    eng.set_data(*splits)
    for g, m in enumerate(members):
        eng.set_model(g, m, 7 if m is model else 11)
    for phase, n in sched:
        eng.eng.begin_phase(phase)
        eng.run(phase, n, lr, 0, use_graph=use_graph)
    eng.eng.sync()
    h = eng.history_rows(slot)
    return eng, np.stack([h[:, HIST["train_loss"]], h[:, HIST["grad_norm"]]], 1).astype(np.float64)


NOISE_ONLY = "sdf_net.output_proj.bias"


def _tensor_errors(sd_gpu, model, steps=None, lr=None):
    """Per-tensor ||gpu - cpu|| / ||cpu||; the noise-only bias is checked here against its bound."""
    out = {}
    for k, v in model.state_dict().items():
        ref = v.detach().double()
        if k == NOISE_ONLY and model.spec.normalize_w and steps is not None:
            assert float((sd_gpu[k].double() - ref).abs().max()) <= 2 * steps * lr * 1.01, k
            continue
        out[k] = float((sd_gpu[k].double() - ref).norm() / max(ref.norm(), 1e-30))
    return out


def _double(b):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}


SCHED = ((1, 2), (2, 4), (3, 3))
LR = 1e-3


def _config(hm=(16,), F=46, M=8, on=True, **upd):
    cfg = default_cli_config(M, F, dropout=0.0, rnn_dim_moment=list(hm), moment_lstm=on)
    cfg.update(upd)
    return cfg


def _model(cfg, seed=0):
    torch.manual_seed(seed)
    return AssetPricingGAN(cfg)


# ---------------------------------------------------------------------------- 1. trajectory
CASES = {
    "csmv16": ((16,), {}),
    "csmv32": ((32,), {}),
    "csmv5": ((5,), {}),
    "csmv16_moment_hidden": ((16,), {"hidden_dim_moment": [16]}),
    "csmv16_no_sdf_lstm": ((16,), {"use_rnn": False}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_matches_cpu_trainer(case):
    """2 unconditional, 4 moment and 3 conditional steps: losses, gradient norms and every parameter
    tensor within 1e-5 of the CPU trainer; where the CPU's fp32 trajectory itself is further than
    that from float64, the GPU is no further from float64 than 2x the CPU plus the same slack."""
    hm, upd = CASES[case]
    splits = _splits()
    model = _model(_config(hm, **upd))
    assert model.spec.moment_rnn_hidden == hm[-1]
    gpu_model, m64 = copy.deepcopy(model), copy.deepcopy(model).double()
    eng, got = _gpu_trajectory(gpu_model, splits, SCHED, LR)
    assert int(eng.desc["mom_H"]) == hm[-1] and int(eng.desc["mom_nrnn"]) == 1
    ref = _cpu_trajectory(model, splits[0], SCHED, LR)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
    errs = _tensor_errors(eng.state_dict(0), model, steps=sum(n for _, n in SCHED), lr=LR)
    worst = max(errs, key=errs.get)
    print(f"{case}: trajectory rel {rel.max(axis=0)}, worst tensor {worst} {errs[worst]:.3g}")
    # the moment LSTM really trained
    init = _model(_config(hm, **upd)).state_dict()
    for k in LSTM_KEYS:
        assert not torch.equal(eng.state_dict(0)[k], init[k]), k
    if rel.max() < TOL and errs[worst] < TOL:
        return
    ref64 = _cpu_trajectory(m64, _double(splits[0]), SCHED, LR)
    e_gpu = np.abs(got - ref64) / np.abs(ref64)
    e_cpu = np.abs(ref - ref64) / np.abs(ref64)
    print(f"{case}: vs float64 gpu {e_gpu.max():.3g} cpu {e_cpu.max():.3g}")
    assert e_gpu.max() <= max(2 * e_cpu.max() + 1e-6, TOL), (case, e_gpu.max(), e_cpu.max(), rel.max(axis=0),
                                                             worst, errs[worst])
    sd64, sdg = m64.state_dict(), eng.state_dict(0)
    for k, v in model.state_dict().items():
        if k == NOISE_ONLY and model.spec.normalize_w:
            continue
        d_gpu = float((sdg[k].double() - sd64[k]).norm() / sd64[k].norm())
        d_cpu = float((v.double() - sd64[k]).norm() / sd64[k].norm())
        assert d_gpu <= 2 * d_cpu + 2 * TOL, (case, k, d_gpu, d_cpu)


# ---------------------------------------------------------------------------- 2. forward table
def _panel(T, N, F, M, seed=0):
    """Train / valid / test splits of T periods each, the macro series standardised over all of
    them (T = 1 has no spread of its own)."""
    ret, feats, mask, mac = generate_panel_fast(3 * T, N, F, M, seed=seed)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    return [{"returns": ret[a:a + T].contiguous(), "individual_features": feats[a:a + T].contiguous(),
             "mask": mask[a:a + T].contiguous(), "macro_features": mac[a:a + T].contiguous()}
            for a in (0, T, 2 * T)]


def _table_ref(model, macro, dtype):
    """abias[T][cm1] = W_m0[:, :Hm] . LSTM(macro) + b_m0 with torch, in ``dtype``."""
    m = copy.deepcopy(model).to(dtype)
    lin = m.moment_net.fc_layers[0] if len(model.spec.moment_hidden) else m.moment_net.output_proj
    Hm = model.spec.moment_rnn_hidden
    with torch.no_grad():
        hm = m.moment_net.encode_macro(macro.to(dtype))
        return (hm @ lin.weight[:, :Hm].T + lin.bias).double().numpy()


def _check_table(model, splits, engines, label):
    cm1 = (list(model.spec.moment_hidden) + [model.spec.num_moments])[0]
    tabs = {}
    for prec, eng in engines.items():
        for s in (0, 1):
            for train_mode in ((False, True) if s == 0 else (False,)):
                eng.eng.forward_split(s, train_mode, True)
                tab = np.asarray(eng.eng.read_ws(0, s, "abias")).reshape(-1, 64)
                T = splits[s]["mask"].shape[0]
                assert tab.shape[0] == T
                assert not tab[:, cm1:].any(), (label, prec, s)
                r64 = _table_ref(model, splits[s]["macro_features"], torch.float64)
                r32 = _table_ref(model, splits[s]["macro_features"], torch.float32)
                e_gpu = np.abs(tab[:, :cm1] - r64).max()
                e_cpu = np.abs(r32 - r64).max()
                print(f"{label} {prec} split {s} train={train_mode}: gpu {e_gpu:.3g} torch fp32 {e_cpu:.3g}")
                assert e_gpu <= 2 * e_cpu + 1e-6, (label, prec, s, train_mode, e_gpu, e_cpu)
                tabs[(prec, s, train_mode)] = tab
    for (prec, s, tm), tab in tabs.items():        # fp32 arithmetic in both engine precisions
        assert np.array_equal(tab, tabs[("fp32", s, tm)]), (label, prec, s, tm)


def _engines(model, splits, precisions=("fp32", "bf16")):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    out = {}
    for prec in precisions:
        eng = GANEngine(model.spec, 1, max_epochs=8, precision=prec)
        eng.set_data(*splits)
        eng.set_model(0, model, 7)
        out[prec] = eng
    return out


@pytest.mark.parametrize("T,M,Hm", [(1, 3, 4), (2, 178, 32), (37, 178, 16), (300, 178, 32)])
def test_forward_table_matches_torch(T, M, Hm):
    """The table within 2x the float32 torch LSTM's own distance from the float64 one, plus 1e-6;
    the bf16 engine's table equals the fp32 engine's bit for bit."""
    splits = _panel(T, 24, 4, M)
    model = _model(_config((Hm,), F=4, M=M))
    _check_table(model, splits, _engines(model, splits), f"T{T}-M{M}-Hm{Hm}")


# ---------------------------------------------------------------------------- 3. long split
def _lstm_grads(model, b, dtype):
    m = copy.deepcopy(model).to(dtype)
    bb = _double(b) if dtype == torch.float64 else b
    o = m(bb["macro_features"], bb["individual_features"], bb["returns"], bb["mask"], phase="moment")
    o["loss"].backward()
    return {k: p.grad.double() for k, p in m.named_parameters() if p.grad is not None}


def _engine_grads(eng, model):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import unflatten_state
    eng.eng.backward_only(2)
    return unflatten_state(np.asarray(eng.eng.get_grads(0)), model.spec)


def test_long_split_beyond_any_staged_limit():
    """T = 1100 at Hm = 32 (the saved gates alone are 563 KB): the forward table as above, and the
    LSTM tensors' gradients of one phase-2 step against autograd by the same criterion -- per
    tensor, no further from the float64 gradient than 2x torch's float32 one, plus 1e-6 at the
    scale of the tensor (its largest float64 element)."""
    splits = _panel(1100, 8, 4, 3)
    model = _model(_config((32,), F=4, M=3))
    engines = _engines(model, splits)
    _check_table(model, splits, engines, "long")
    got = _engine_grads(engines["fp32"], model)
    g64, g32 = _lstm_grads(model, splits[0], torch.float64), _lstm_grads(model, splits[0], torch.float32)
    for k in LSTM_KEYS:
        scale = float(g64[k].abs().max())
        e_gpu = float((got[k].double() - g64[k]).abs().max())
        e_cpu = float((g32[k] - g64[k]).abs().max())
        print(f"long {k}: gpu {e_gpu:.3g} torch fp32 {e_cpu:.3g} scale {scale:.3g}")
        assert scale > 0
        assert e_gpu <= 2 * e_cpu + 1e-6 * scale, (k, e_gpu, e_cpu, scale)


# ---------------------------------------------------------------------------- 4. backward alone
@pytest.mark.parametrize("case", ["csmv16", "csmv32", "csmv5", "csmv16_moment_hidden"])
def test_phase2_gradients_match_autograd(case):
    """One phase-2 backward at the trajectory shape, one whole period of the train split masked (its
    dab row is zero; it still has a state): every moment-network tensor's gradient within 1e-5 of
    autograd on the CPU model, relative to that tensor's norm."""
    hm, upd = CASES[case]
    splits = _splits()
    splits[0]["mask"][7] = False
    model = _model(_config(hm, **upd))
    eng = _engines(model, splits, ("fp32",))["fp32"]
    got = _engine_grads(eng, model)
    ref = _lstm_grads(model, splits[0], torch.float32)
    seen = 0
    for k, _ in model.spec.param_layout():
        if not k.startswith("moment_net."):
            continue
        err = float((got[k].double() - ref[k]).norm() / ref[k].norm())
        print(f"{case} {k}: {err:.3g}")
        assert err < TOL, (case, k, err)
        seen += 1
    assert seen == 4 + 2 * (1 + len(model.spec.moment_hidden))


# ---------------------------------------------------------------------------- 5. determinism
def _final(eng, g=0):
    return np.asarray(eng.params(g)).copy(), np.asarray(eng.history_rows(g)).copy()


def test_determinism_and_invariance():
    splits = _splits()
    cfg = _config((16,))
    a, b = _model(cfg, 0), _model(cfg, 1)
    p0, h0 = _final(_gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR)[0])
    p1, h1 = _final(_gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR)[0])
    assert np.array_equal(p0, p1) and np.array_equal(h0, h1, equal_nan=True)
    p2, h2 = _final(_gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR, use_graph=False)[0])
    assert np.array_equal(p0, p2) and np.array_equal(h0, h2, equal_nan=True)
    for slot in (0, 1):
        eng, _ = _gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR, others=[copy.deepcopy(b)], slot=slot)
        p3, h3 = _final(eng, slot)
        assert np.array_equal(p0, p3) and np.array_equal(h0, h3, equal_nan=True), slot
        assert not np.array_equal(p0, _final(eng, 1 - slot)[0])
    q0, g0 = _final(_gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR, precision="bf16")[0])
    q1, g1 = _final(_gpu_trajectory(copy.deepcopy(a), splits, SCHED, LR, precision="bf16")[0])
    assert np.isfinite(q0).all() and np.isfinite(g0[:, 1]).all()
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1, equal_nan=True)


# ---------------------------------------------------------------------------- 6. bf16 gap
def test_bf16_gap_no_wider_than_without_the_lstm():
    """After the schedule's four phase-2 steps: |moment loss (bf16 engine) - moment loss (fp32
    engine)| with the feature on is at most twice the same difference for the same config with it
    off -- the towers round identically in both, the LSTM adds fp32 work only."""
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import HIST
    splits = _splits()
    sched = SCHED[:2]
    gap = {}
    for on in (False, True):
        model = _model(_config((16,), on=on))
        loss = {}
        for prec in ("fp32", "bf16"):
            eng, _ = _gpu_trajectory(copy.deepcopy(model), splits, sched, LR, precision=prec)
            h = eng.history_rows(0)
            assert int(h[-1, HIST["phase"]]) == 2
            loss[prec] = float(h[-1, HIST["train_loss"]])
        gap[on] = abs(loss["bf16"] - loss["fp32"])
        print(f"moment_lstm={on}: fp32 {loss['fp32']:.9g} bf16 {loss['bf16']:.9g} gap {gap[on]:.3g}")
    out_dir = os.environ.get("DLAP_PROFILE_DIR")      # (set to record profiles/moment_lstm_accuracy.txt)
    if out_dir:
        with open(os.path.join(out_dir, "moment_lstm_accuracy.txt"), "w") as fh:
            fh.write("bf16 engine vs fp32 engine, moment loss after 2 unconditional + 4 moment steps\n"
                     "(T = 36/12/18, N = 160, F = 46, M = 8, CSMV 16, dropout 0)\n"
                     f"moment_lstm off: |bf16 - fp32| = {gap[False]:.6g}\n"
                     f"moment_lstm on:  |bf16 - fp32| = {gap[True]:.6g}  (bound: 2x off = {2 * gap[False]:.6g})\n")
    assert gap[True] <= 2 * gap[False], gap


# ---------------------------------------------------------------------------- 7. plan and limits
def test_plan_and_limits(monkeypatch):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    splits = _splits()
    info = {}
    for on in (False, True):
        model = _model(_config((16,), on=on))
        eng = GANEngine(model.spec, 1, max_epochs=8, precision="fp32")
        eng.set_data(*splits)
        eng.set_model(0, model, 7)
        eng.run(2, 1, LR, 0)
        eng.eng.sync()
        info[on] = dict(eng.eng.fused_info())
        if on:
            with pytest.raises(ValueError, match="set_xs"):
                eng.eng.set_xs(lambda *a: None)
    assert info[True]["mom_tail"] is False
    assert info[False]["mom_tail"] is True            # unchanged without the key
    same = [k for k in info[False] if k not in ("mom_tail", "host_launch_us_per_epoch")]
    assert {k: info[True][k] for k in same} == {k: info[False][k] for k in same}
    nat = native.load(required=True)
    kw = dict(F=46, M=8, nrnn=1, H=4, raw_macro_sdf=False, hidden=[64, 64], mom_hidden=[], K=8, dropout=0.0,
              normalize_w=True, weighted=True, residual=0.0, G=1, max_epochs=4, fp32=True)
    with pytest.raises(ValueError, match="exactly 1 layer"):
        nat.Engine(**kw, mom_nrnn=2, mom_H=16)
    with pytest.raises(ValueError, match=r"\[1, 32\]"):
        nat.Engine(**kw, mom_nrnn=1, mom_H=33)
    with pytest.raises(ValueError, match="M >= 1"):
        nat.Engine(**dict(kw, M=0, nrnn=0), mom_nrnn=1, mom_H=16)
    monkeypatch.setenv("DLAP_WIDE", "1")
    with pytest.raises(ValueError, match="wide layer-0 path"):
        nat.Engine(**kw, mom_nrnn=1, mom_H=16)
    monkeypatch.delenv("DLAP_WIDE")
    with pytest.raises(ValueError, match="wide layer-0 path"):      # wide by size
        nat.Engine(**dict(kw, F=200), mom_nrnn=1, mom_H=16)


def test_module_forward_on_cuda_matches_cpu(capsys):
    b = _splits()[0]
    model = _model(_config((16,)))
    with torch.no_grad():
        ref = model(b["macro_features"], b["individual_features"], b["returns"], b["mask"], phase="moment")
        w_ref, _ = model.get_weights(b["macro_features"], b["individual_features"], b["mask"], normalized=True)
    g = copy.deepcopy(model).cuda()
    bc = {k: v.cuda() for k, v in b.items()}
    with torch.no_grad():
        out = g(bc["macro_features"], bc["individual_features"], bc["returns"], bc["mask"], phase="moment")
        w, _ = g.get_weights(bc["macro_features"], bc["individual_features"], bc["mask"], normalized=True)
    for k in ("weights", "moments", "loss", "loss_conditional", "portfolio_returns"):
        a, r = out[k].cpu().double(), ref[k].double()
        assert float((a - r).abs().max()) <= TOL * max(float(r.abs().max()), 1e-30), k
    assert float((w.cpu() - w_ref).abs().max()) <= TOL * float(w_ref.abs().max())


# ---------------------------------------------------------------------------- 8. full schedule
def test_train_3phase_matches_cpu():
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import train_3phase_gpu
    from deeplearninginassetpricing_paperreplication_amd.train.trainer import _train_3phase_cpu
    tr, va, te = _splits()
    cfg = _config((16,))
    m_cpu = _model(cfg)
    m_gpu = copy.deepcopy(m_cpu)
    kw = dict(num_epochs_unc=6, num_epochs_moment=3, num_epochs=6, lr=1e-3, print_freq=100, ignore_epoch=1)
    m_gpu, h_gpu = train_3phase_gpu(cfg, tr, va, te, device="cuda", precision="fp32", selection_sign=1.0,
                                    verbose=False, models=[m_gpu], seeds=[7], **kw)
    m_cpu, h_cpu = _train_3phase_cpu(cfg, tr, va, te, torch.device("cpu"), kw["num_epochs_unc"],
                                     kw["num_epochs_moment"], kw["num_epochs"], kw["lr"], 100, None,
                                     kw["ignore_epoch"], 1.0, False, model=m_cpu)
    assert h_gpu["phase"] == h_cpu["phase"]
    for k in ("train_loss", "valid_loss", "test_loss"):
        a, b = np.asarray(h_gpu[k]), np.asarray(h_cpu[k])
        assert np.abs(a - b).max() <= TOL * np.abs(b).max(), k
    for k in ("train_sharpe", "valid_sharpe", "test_sharpe"):
        a, b = np.asarray(h_gpu[k]), np.asarray(h_cpu[k])
        assert np.abs(a - b).max() < 1e-4, (k, a, b)
    errs = _tensor_errors({k: v.cpu() for k, v in m_gpu.state_dict().items()}, m_cpu,
                          steps=kw["num_epochs_unc"] + kw["num_epochs"], lr=kw["lr"])
    worst = max(errs, key=errs.get)
    assert errs[worst] < TOL, (worst, errs[worst])
    init = _model(cfg).state_dict()
    for k in LSTM_KEYS:
        assert not torch.equal(m_gpu.state_dict()[k].cpu(), init[k]), k

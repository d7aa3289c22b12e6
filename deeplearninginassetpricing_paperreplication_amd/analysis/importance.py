"""Variable importance of the SDF weight (the paper's sensitivity ranking).

    Sens(x_j) = (1/C) * sum_t sum_i | d w(I_t, I_{t,i}) / d x_j |      (normalised to sum to one)

for every input column of the SDF tower: the F firm characteristics and the Dm "state" columns a
row's period contributes (the LSTM output of the macro series, or the raw macro series when the
model has no LSTM). ``w`` is the ensemble weight: the average over the models of their scaled raw
tower outputs, so the members' gradients are summed WITH their signs per row before the absolute
value is taken.

Two scales of model g's output in period t:
  ``"raw"``       s = 1/G: the plain average of the raw tower outputs;
  ``"ensemble"``  s[g][t] = 1 / (G * sum_i |wn_{g,t,i}|), wn the model's (zero-mean) weights: the
                  direct-effect gradient of the averaged L1-normalised weight that
                  ``evaluate_ensemble`` forms. The per-period mean and L1 norm are treated as
                  constants -- the indirect effect of one stock's characteristic on the other
                  stocks' weights through the normalisation is not part of the ranking.

``device="cpu"`` differentiates the PyTorch tower with autograd (any architecture).
``device="cuda"`` runs the native engine's input-gradient kernel (``csrc/k_sens.hip``), one launch
for all models of the ensemble; mixed-architecture ensembles and shapes the kernel does not cover
(the wide layer-0 path) fall back to the CPU path with a printed note.

Macro importance through the LSTM (``macro_lags = L > 0``). ``m`` is the standardised macro series
the model is fed (``batch["macro_features"]``), ``w`` the ensemble weight with the same ``scale``
semantics (members summed with their signs per row before the absolute value). The split's
recurrence starts from the engine's ``h0 / c0`` (zero unless set), and macro values before the
split's first period are constants. For the lags ``l = 0 .. L-1`` (``L`` clamped to ``T``):

    macro_lag[l][j] = (1 / rows_lag[l]) * sum over valid rows (t,i), t >= l, of
                          | sum_g s_g,t * d w_g(t,i) / d m[t-l][j] |
    macro_cum[j]    = (1 / rows) * sum over valid rows of
                          | sum_{l < min(L, t+1)} sum_g s_g,t * d w_g(t,i) / d m[t-l][j] |

``rows_lag[l]`` is the number of valid rows in the periods ``t >= l``; ``macro`` is ``macro_lag[0]``
normalised to sum to one (the current-month ranking of the paper's macro figure) and ``macro_cum``
the response to a shift of series ``j`` sustained over the window. The dependence on the macro
history factors through the state columns,

    d w_g(t,i) / d m[t-l][j] = sum_k d_g(t,i)[k] * J_g[t][l][k][j],   J_g[t][l] = d h_t / d m_{t-l},

so it is a per-period Jacobian times the per-row state gradient, not a per-row BPTT. The CPU path
takes ``J`` from autograd of ``macro_lstm`` (any depth); the engine (``csrc/k_macro_sens.hip``)
covers single-layer LSTMs of up to 8 units on the fused layer-0 path and everything else falls
back to the CPU path. Without an LSTM the state columns are the macro series: ``macro_lag[0]`` is
the state-column result and the higher lags are zero.

Out of scope: per-period breakdowns, the moment network, and the indirect effect through the
weight normalisation.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..models import losses as L


def _state(model, macro):
    """The per-period columns of the tower input: LSTM(macro) [T, H], raw macro [T, M], or None."""
    net = model.sdf_net
    if macro is None:
        return None
    if net.macro_lstm is not None:
        with torch.no_grad():
            return net.macro_lstm(macro)[0]
    return macro


def _has_lstm(model) -> bool:
    return model.sdf_net.macro_lstm is not None


def input_names(F: int, Dm: int, lstm: bool, names: Optional[Sequence] = None) -> List[str]:
    ch = [str(n) for n in names] if names is not None and len(names) == F else [f"x{j}" for j in range(F)]
    return ch + [f"{'state' if lstm else 'macro'}{j}" for j in range(Dm)]


def _model_scale(w_raw, mask, normalize: bool, G: int, scale: str):
    """[Tc] scale of one model's gradient for the periods of w_raw [Tc, N]."""
    if scale == "raw":
        return torch.full((w_raw.shape[0],), 1.0 / G, dtype=w_raw.dtype)
    wn = L.zero_mean_normalize(w_raw, mask) if normalize else w_raw * mask.to(w_raw.dtype)
    return 1.0 / (G * (wn.abs() * mask.to(w_raw.dtype)).sum(dim=1).clamp(min=1e-8))


def _cpu_sums(models, batch, scale: str, dtype, chunk: int = 16) -> Dict:
    """abs [G, C], sum [G, C], ens [C] (float64) and rows over the valid rows of the batch."""
    feats = batch["individual_features"].to(dtype)
    mask = batch["mask"].bool()
    macro = batch.get("macro_features")
    macro = None if macro is None else macro.to(dtype)
    T, N, F = feats.shape
    G = len(models)
    ms = [copy.deepcopy(m).to(dtype).eval() for m in models]
    states = [_state(m, macro) for m in ms]
    dms = {0 if s is None else int(s.shape[-1]) for s in states}
    if len(dms) != 1:
        raise ValueError("variable_importance: the models' state widths differ")
    Dm = dms.pop()
    C = F + Dm
    ab = np.zeros((G, C)); sm = np.zeros((G, C)); ens = np.zeros(C)
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        mk = mask[t0:t1]
        tot = torch.zeros(t1 - t0, N, C, dtype=torch.float64)
        for g, m in enumerate(ms):
            x = feats[t0:t1].clone().requires_grad_(True)
            leaves = [x]
            if Dm:
                st = states[g][t0:t1, None, :].expand(t1 - t0, N, Dm).clone().requires_grad_(True)
                leaves.append(st)
            inp = torch.cat(leaves, -1)
            net = m.sdf_net
            w_raw = net.output_proj(net.fc_layers(inp.reshape(-1, C))).reshape(t1 - t0, N)
            grads = torch.autograd.grad(w_raw.sum(), leaves)
            s = _model_scale(w_raw.detach(), mk, net.normalize_weights, G, scale)
            dx = torch.cat(grads, -1).double() * s.double()[:, None, None] * mk[:, :, None].double()
            ab[g] += dx.abs().sum((0, 1)).numpy()
            sm[g] += dx.sum((0, 1)).numpy()
            tot += dx
        ens += tot.abs().sum((0, 1)).numpy()
    return {"abs": ab, "sum": sm, "ens": ens, "rows": int(mask.sum()), "F": F, "Dm": Dm}


def _lag_jacobians(lstm, macro, L: int):
    """J [T, L, H, M] = d h_t / d m_{t-l} of ``macro_lstm`` (zero where t - l < 0): per period the
    H unit seeds are carried back by autograd (batched where the LSTM backward supports it)."""
    m = macro.detach().clone().requires_grad_(True)
    h = lstm(m)[0]
    T, H = h.shape
    J = torch.zeros(T, L, H, m.shape[1], dtype=macro.dtype)
    eye = torch.eye(H, dtype=h.dtype)
    batched = True
    for t in range(T):
        g = None
        if batched:
            try:
                g = torch.autograd.grad(h[t], m, grad_outputs=eye, is_grads_batched=True, retain_graph=True)[0]
            except RuntimeError:
                batched = False
        if g is None:
            g = torch.stack([torch.autograd.grad(h[t, k], m, retain_graph=True)[0] for k in range(H)])
        n = min(L, t + 1)
        J[t, :n] = g[:, t - n + 1:t + 1].flip(1).permute(1, 0, 2)      # lag l is period t - l
    return J


def _cpu_macro(models, batch, scale: str, dtype, lags: int) -> Dict:
    """m_abs [G, L, M], m_ens [L, M], m_cum [M] (float64): the per-row state gradients contracted
    with the per-period lag Jacobians of every model's LSTM, in period chunks."""
    feats = batch["individual_features"].to(dtype)
    mask = batch["mask"].bool()
    macro = batch["macro_features"].to(dtype)
    T, N, F = feats.shape
    M = int(macro.shape[1])
    G, Lg = len(models), min(int(lags), T)
    ms = [copy.deepcopy(m).to(dtype).eval() for m in models]
    if not all(_has_lstm(m) for m in ms):
        raise ValueError("variable_importance: macro lags need an LSTM in every model")
    states = [_state(m, macro) for m in ms]
    if len({int(s.shape[-1]) for s in states}) != 1:
        raise ValueError("variable_importance: the models' state widths differ")
    Dm = int(states[0].shape[-1])
    jac = [_lag_jacobians(m.sdf_net.macro_lstm, macro, Lg).double() for m in ms]
    ab = np.zeros((G, Lg, M)); ens = np.zeros((Lg, M)); cum = np.zeros(M)
    chunk = max(1, min(16, int(4e6 // max(N * Lg * M, 1))))
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        mk = mask[t0:t1]
        tot = torch.zeros(Lg, t1 - t0, N, M, dtype=torch.float64)
        for g, m in enumerate(ms):
            st = states[g][t0:t1, None, :].expand(t1 - t0, N, Dm).clone().requires_grad_(True)
            net = m.sdf_net
            w_raw = net.output_proj(net.fc_layers(torch.cat([feats[t0:t1], st], -1).reshape(-1, F + Dm)))
            w_raw = w_raw.reshape(t1 - t0, N)
            ds = torch.autograd.grad(w_raw.sum(), st)[0]
            s = _model_scale(w_raw.detach(), mk, net.normalize_weights, G, scale)
            d = ds.double() * s.double()[:, None, None] * mk[:, :, None].double()
            p = torch.einsum("tik,tlkj->ltij", d, jac[g][t0:t1])
            ab[g] += p.abs().sum((1, 2)).numpy()
            tot += p
        ens += tot.abs().sum((1, 2)).numpy()
        cum += tot.sum(0).abs().sum((0, 1)).numpy()
    return {"m_abs": ab, "m_ens": ens, "m_cum": cum}


def _gpu_sums(models, batch, scale: str, macro_lags: int = 0) -> Optional[Dict]:
    """The same sums from the native engine, or None (with a printed note) where it does not apply."""
    specs = {m.spec for m in models}
    if len(specs) != 1:
        print("[importance] mixed-architecture ensemble: using the CPU path")
        return None
    from ..engine.runner import GANEngine
    spec = models[0].spec
    G = len(models)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = GANEngine(spec, G, max_epochs=4)
    eng.set_data(batch)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    e = eng.eng
    T, N = batch["mask"].shape
    try:
        if scale == "raw":
            sc = torch.full((G, T), 1.0 / G, dtype=torch.float32, device=dev)
            refresh = True
        else:
            ts = torch.cuda.current_stream(dev).cuda_stream
            wn = torch.empty(G, T, N, dtype=torch.float32, device=dev)
            e.join_from(ts)
            e.forward_split(0, False, False)
            for g in range(G):
                e.copy_ws(g, 0, "wn", wn[g].data_ptr())
            e.join_to(ts)
            sc = (1.0 / (G * wn.abs().sum(dim=2).clamp(min=1e-8))).contiguous()
            refresh = False
        torch.cuda.synchronize(dev)
        mr = None
        try:
            r = e.input_sensitivity(0, sc.data_ptr(), refresh)
            if macro_lags > 0 and _has_lstm(models[0]):      # (the forward above left the state current)
                mr = e.macro_sensitivity(0, sc.data_ptr(), int(macro_lags), False)
        except ValueError as err:
            print(f"[importance] {err}: using the CPU path")
            return None
    finally:
        e.sync()
    F = spec.individual_dim
    out = {"abs": np.asarray(r["abs"]), "sum": np.asarray(r["sum"]), "ens": np.asarray(r["ens"]),
           "rows": int(r["rows"]), "F": F, "Dm": int(np.asarray(r["ens"]).shape[0]) - F}
    if mr is not None:
        out.update(m_abs=np.asarray(mr["abs"]), m_ens=np.asarray(mr["ens"]), m_cum=np.asarray(mr["cum"]))
    return out


def _unit(v: np.ndarray) -> np.ndarray:
    s = float(v.sum())
    return v / s if s > 0 else v


def _macro_result(r: Dict, mask, lags: int, lstm: bool, G: int, macro_names: Optional[Sequence]) -> Dict:
    """The macro keys of the result from the raw sums (m_* with an LSTM, else the state columns)."""
    per = mask.bool().sum(1).cpu().numpy().astype(np.int64)
    T = int(per.shape[0])
    Lg = min(int(lags), T)
    rows_lag = np.array([int(per[l:].sum()) for l in range(Lg)], dtype=np.int64)
    den = np.maximum(rows_lag, 1).astype(np.float64)
    rows = max(int(r["rows"]), 1)
    if lstm:
        m_abs, m_ens, m_cum = r["m_abs"], r["m_ens"], r["m_cum"]
    else:                                   # the state columns are the macro series themselves
        F, Dm = r["F"], r["Dm"]
        m_abs = np.zeros((G, Lg, Dm)); m_ens = np.zeros((Lg, Dm))
        m_abs[:, 0] = r["abs"][:, F:]
        m_ens[0] = r["ens"][F:]
        m_cum = np.array(r["ens"][F:], dtype=np.float64)
    M = int(m_ens.shape[1])
    lag = m_ens / den[:, None]
    nm = [str(n) for n in macro_names] if macro_names is not None and len(macro_names) == M \
        else [f"macro{j}" for j in range(M)]
    return {"macro": _unit(lag[0]), "macro_lag": lag, "macro_cum": m_cum / rows,
            "per_model_macro_lag": m_abs / den[None, :, None], "rows_lag": rows_lag, "macro_names": nm}


def variable_importance(models: Sequence, batch: Dict, device: str = "cpu", scale: str = "ensemble",
                        dtype: torch.dtype = torch.float32, names: Optional[Sequence] = None,
                        macro_lags: int = 0, macro_names: Optional[Sequence] = None) -> Dict:
    """Sensitivity of the ensemble SDF weight to every tower input column over ``batch``.

    Returns ``characteristics`` [F] and ``state`` [Dm] (mean absolute gradient of the ensemble
    weight, each block normalised to sum to one), ``abs_mean`` [C] (the same, not normalised),
    ``per_model_abs_mean`` / ``per_model_signed_mean`` [G][C] and ``names`` (``names`` when given
    for the characteristics, otherwise x0.., then state0.. or macro0.. without an LSTM).

    ``scale="ensemble"`` is the direct-effect gradient of the averaged L1-normalised weight: each
    model's per-period mean and L1 norm are held constant (see the module docstring).
    ``dtype`` applies to the CPU path; the engine computes in its own precision.

    ``macro_lags = L > 0`` adds the importance of the macro series through the LSTM (module
    docstring): ``macro`` [M], ``macro_lag`` [L][M], ``macro_cum`` [M], ``per_model_macro_lag``
    [G][L][M], ``rows_lag`` [L] and ``macro_names`` (``macro_names`` when given, else macro0..);
    ``L`` is clamped to the number of periods. ``0`` leaves the result as it is without it.
    """
    if scale not in ("ensemble", "raw"):
        raise ValueError("scale must be 'ensemble' or 'raw'")
    if int(macro_lags) < 0:
        raise ValueError("macro_lags must be >= 0")
    macro_lags = int(macro_lags)
    models = list(models)
    if not models:
        raise ValueError("no models")
    lstm = _has_lstm(models[0])
    r = None
    if str(device).startswith("cuda"):
        r = _gpu_sums(models, batch, scale, macro_lags)
    if r is None:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        cms = [m.cpu() if hasattr(m, "cpu") else m for m in models]
        r = _cpu_sums(cms, cpu, scale, dtype)
        if macro_lags > 0 and lstm:
            r.update(_cpu_macro(cms, cpu, scale, dtype, macro_lags))
    F, Dm, rows = r["F"], r["Dm"], max(int(r["rows"]), 1)
    mean = r["ens"] / rows
    out = {
        "characteristics": _unit(mean[:F]), "state": _unit(mean[F:]), "abs_mean": mean,
        "per_model_abs_mean": r["abs"] / rows, "per_model_signed_mean": r["sum"] / rows,
        "names": input_names(F, Dm, lstm, names), "rows": int(r["rows"]),
    }
    if macro_lags > 0:
        out.update(_macro_result(r, batch["mask"], macro_lags, lstm, len(models), macro_names))
    return out


def format_importance(imp: Dict, top: int = 20) -> List[str]:
    """The printed report: the top characteristics and every state column."""
    F = len(imp["characteristics"])
    names = imp["names"]
    order = np.argsort(-imp["characteristics"])[:top]
    lines = [f"  Top {len(order)} characteristics (share of the mean |dw/dx|):"]
    lines += [f"    {k + 1:2d}. {names[j]:<16s} {imp['characteristics'][j]:.4f}" for k, j in enumerate(order)]
    if len(imp["state"]):
        lines.append("  State columns:")
        lines += [f"        {names[F + j]:<16s} {imp['state'][j]:.4f}" for j in range(len(imp["state"]))]
    if "macro" in imp and len(imp["macro"]):
        mo = np.argsort(-imp["macro"])[:top]
        lines.append(f"  Top {len(mo)} macro series (share of the mean |dw/dm| at lag 0; sustained over "
                     f"{len(imp['macro_lag'])} lag(s)):")
        lines += [f"    {k + 1:2d}. {imp['macro_names'][j]:<16s} {imp['macro'][j]:.4f}   {imp['macro_cum'][j]:.3e}"
                  for k, j in enumerate(mo)]
    return lines


def to_json(imp: Dict) -> Dict:
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in imp.items()}

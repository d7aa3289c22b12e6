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

Out of scope: the importance of the raw macro series THROUGH the LSTM (a per-row BPTT), per-period
breakdowns, and the moment network.
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


def _gpu_sums(models, batch, scale: str) -> Optional[Dict]:
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
        try:
            r = e.input_sensitivity(0, sc.data_ptr(), refresh)
        except ValueError as err:
            print(f"[importance] {err}: using the CPU path")
            return None
    finally:
        e.sync()
    F = spec.individual_dim
    return {"abs": np.asarray(r["abs"]), "sum": np.asarray(r["sum"]), "ens": np.asarray(r["ens"]),
            "rows": int(r["rows"]), "F": F, "Dm": int(np.asarray(r["ens"]).shape[0]) - F}


def _unit(v: np.ndarray) -> np.ndarray:
    s = float(v.sum())
    return v / s if s > 0 else v


def variable_importance(models: Sequence, batch: Dict, device: str = "cpu", scale: str = "ensemble",
                        dtype: torch.dtype = torch.float32, names: Optional[Sequence] = None) -> Dict:
    """Sensitivity of the ensemble SDF weight to every tower input column over ``batch``.

    Returns ``characteristics`` [F] and ``state`` [Dm] (mean absolute gradient of the ensemble
    weight, each block normalised to sum to one), ``abs_mean`` [C] (the same, not normalised),
    ``per_model_abs_mean`` / ``per_model_signed_mean`` [G][C] and ``names`` (``names`` when given
    for the characteristics, otherwise x0.., then state0.. or macro0.. without an LSTM).

    ``scale="ensemble"`` is the direct-effect gradient of the averaged L1-normalised weight: each
    model's per-period mean and L1 norm are held constant (see the module docstring).
    ``dtype`` applies to the CPU path; the engine computes in its own precision.
    """
    if scale not in ("ensemble", "raw"):
        raise ValueError("scale must be 'ensemble' or 'raw'")
    models = list(models)
    if not models:
        raise ValueError("no models")
    r = None
    if str(device).startswith("cuda"):
        r = _gpu_sums(models, batch, scale)
    if r is None:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        r = _cpu_sums([m.cpu() if hasattr(m, "cpu") else m for m in models], cpu, scale, dtype)
    F, Dm, rows = r["F"], r["Dm"], max(int(r["rows"]), 1)
    mean = r["ens"] / rows
    return {
        "characteristics": _unit(mean[:F]), "state": _unit(mean[F:]), "abs_mean": mean,
        "per_model_abs_mean": r["abs"] / rows, "per_model_signed_mean": r["sum"] / rows,
        "names": input_names(F, Dm, _has_lstm(models[0]), names), "rows": int(r["rows"]),
    }


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
    return lines


def to_json(imp: Dict) -> Dict:
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in imp.items()}

"""Prediction towers: the FFN return-prediction benchmark and the beta network of the paper's
main table. Both fit a tower of the SDF network's architecture (LSTM state + characteristics ->
one scalar per row, the raw output: no zero-mean normalisation) by mean squared error to a per-row
target ``y[t,i] = R[t,i] f[t]``; the FFN benchmark uses ``f = 1``, the beta network the SDF factor.

Definition. For a split with valid rows ``r = (t, i)``, raw tower output ``p`` (float32), returns
``R`` (float32) and an optional ``f[t]`` (float32; absent: 1)::

    y = fp32(R * f[t])                      e = fp32(p - y)
    per period t, float64 sums over its valid rows:
      n, SE = sum e^2, SY = sum y^2, S1 = sum p, SA = sum |p|, S2 = sum p^2, SR = sum p R
    weighting "period" (default):  c[t] = fp32(1 / (T' n_t)),  T' = periods with n_t > 0
    weighting "pooled":            c[t] = fp32(1 / R_total)
    loss = sum_t float64(c[t]) * SE[t]      dw[r] = 2 c[t] e   (float32, one rounding)

Empty periods contribute nothing; a split without rows has loss 0. Everything downstream follows
from the sums (``metrics_from_sums``, the algebra of ``benchmarks.factors_from_sums`` /
``ev_from_sums`` with ``v = p``): the factor ``F_t = SR / SA`` (``SR`` where ``SA <= 1e-8``), its
Sharpe ratio, EV with loadings ``p`` and the prediction R² ``1 - sum SE / sum SY``. The loss of the
zero predictor is ``sum_t c[t] SY[t]``.

A fit epoch is one full-batch step: train-mode forward of the train split, the loss above and its
gradient, ``clip_grad_norm_`` (1.0) and Adam (the trainer's settings) over the parameters phase 1
trains (``sdf_net``), then the evaluation-mode loss of the validation and test splits with the
updated parameters. Each tower is selected at its first best validation epoch (strictly lower
loss; NaN never wins); the predictions of several seeds are averaged.

``device="cpu"`` runs the loop in torch (the oracle of the trajectory). ``device="cuda"`` runs all
seeds batched in one native engine (``Engine.fit_begin`` / ``fit_epochs``: ``csrc/k_pred.hip`` for the
loss and the bookkeeping, the engine's own forward / backward / Adam kernels for the rest), with no
host round trip between epochs. With dropout the two devices draw different masks; with dropout 0
and ``precision="fp32"`` they follow the same trajectory to 1e-5.

Out of scope: graph capture of the fit epoch, cross-sectional sharding and multi-rank fits,
hyperparameter search for the FFN, value weighting, plots.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .portfolio import cross_sectional_r2, explained_variation, renormalize, sharpe_ddof0

SPLITS = ("train", "valid", "test")
SUMS = ("se", "sy", "s1", "sa", "s2", "sr")
HIST = dict(train_loss=0, valid_loss=1, test_loss=2, grad_norm=3, best=4)
GRAD_CLIP = 1.0


def _np(a, dtype=None) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)


def row_weights(mask, weighting: str = "period") -> np.ndarray:
    """``c [T]`` float32 of the weighting (0 for an empty period under "period")."""
    m = _np(mask).astype(bool)
    n = m.sum(axis=1).astype(np.float64)
    if weighting == "pooled":
        tot = n.sum()
        return np.full(m.shape[0], np.float32(1.0 / tot) if tot > 0 else np.float32(0.0), dtype=np.float32)
    if weighting != "period":
        raise ValueError("weighting must be 'period' or 'pooled'")
    tp = float((n > 0).sum())
    return np.where(n > 0, 1.0 / np.maximum(tp * n, 1.0), 0.0).astype(np.float32)


def prediction_sums_numpy(pred, returns, mask, factor=None, weighting: str = "period", grad: bool = False) -> Dict:
    """The definition above on dense ``pred``, ``returns``, ``mask`` [T][N] and ``factor`` [T] or
    None: ``n`` int32 [T], ``se`` .. ``sr`` float64 [T], ``c`` float32 [T], ``loss`` and
    ``loss_zero`` (the zero predictor's); with ``grad`` also ``dw`` float32 [T][N] (0 at the invalid
    entries)."""
    p, r, m = _np(pred, np.float32), _np(returns, np.float32), _np(mask).astype(bool)
    T, N = m.shape
    f = np.ones(T, np.float32) if factor is None else _np(factor, np.float32).reshape(T)
    c = row_weights(m, weighting)
    y = (r * f[:, None]).astype(np.float32)
    e = (p - y).astype(np.float32)
    md = m.astype(np.float64)
    pd, ed, yd, rd = (a.astype(np.float64) * md for a in (p, e, y, r))
    out = {"n": m.sum(axis=1).astype(np.int32), "se": (ed * ed).sum(axis=1), "sy": (yd * yd).sum(axis=1),
           "s1": pd.sum(axis=1), "sa": np.abs(pd).sum(axis=1), "s2": (pd * pd).sum(axis=1),
           "sr": (pd * rd).sum(axis=1), "c": c}
    out["loss"] = float((c.astype(np.float64) * out["se"]).sum())
    out["loss_zero"] = float((c.astype(np.float64) * out["sy"]).sum())
    if grad:
        out["dw"] = np.where(m, (np.float32(2.0) * c)[:, None] * e, np.float32(0.0)).astype(np.float32)
    return out


def metrics_from_sums(sums: Dict, returns, mask) -> Dict:
    """Factor [T], its Sharpe ratio, EV with loadings ``p`` and the prediction R² from the
    per-period sums of one model (``sum_rr`` comes from the panel)."""
    from .benchmarks import ev_from_sums, factors_from_sums
    r, m = _np(returns, np.float64), _np(mask).astype(bool)
    s = {"sa": np.asarray(sums["sa"])[:, None], "sr": np.asarray(sums["sr"])[:, None],
         "s2": np.asarray(sums["s2"])[:, None], "n": np.asarray(sums["n"]), "sum_rr": (r * r * m).sum(axis=1)}
    f = factors_from_sums(s)[:, 0]
    sy = float(np.asarray(sums["sy"]).sum())
    return {"factor": f, "sharpe": sharpe_ddof0(f), "ev": float(ev_from_sums(s)[0]),
            "r2": 1.0 - float(np.asarray(sums["se"]).sum()) / sy if sy > 0 else float("nan")}


# ---------------------------------------------------------------------------------------------
# The fit

def _names(batches: Dict[str, Dict]) -> List[str]:
    for s in ("train", "valid"):
        if s not in batches:
            raise ValueError("batches must hold 'train' and 'valid' (and optionally 'test')")
    return [s for s in SPLITS if s in batches]


def _factor_of(factor, name: str, T: int) -> Optional[np.ndarray]:
    if factor is None or factor.get(name) is None:
        return None
    f = np.ascontiguousarray(_np(factor[name], np.float32).reshape(-1))
    if f.shape[0] != T:
        raise ValueError(f"factor[{name!r}] must be [{T}]")
    return f


def _raw_output(model, batch, dtype=torch.float32):
    """Raw tower output [T][N] of ``model.sdf_net`` (with grad: the LSTM state as
    ``importance._state`` forms it, the tower as ``weight_structure._tower``)."""
    from .weight_structure import _tower
    net = model.sdf_net
    feats = batch["individual_features"].to(dtype)
    macro = batch.get("macro_features")
    state = None if macro is None else macro.to(dtype)
    if state is not None and net.macro_lstm is not None:
        state = net.macro_lstm(state)[0]
    T, N, _ = feats.shape
    x = feats if state is None else torch.cat([feats, state[:, None, :].expand(T, N, state.shape[-1])], -1)
    return _tower(model, x.reshape(T * N, -1)).reshape(T, N)


def _torch_loss(p, batch, f, c):
    m = batch["mask"].bool()
    y = batch["returns"].to(p.dtype) if f is None else batch["returns"].to(p.dtype) * f[:, None]
    e = torch.where(m, p - y, torch.zeros((), dtype=p.dtype))
    return (c * (e * e).sum(dim=1)).sum()


def _tensor_batch(b: Dict) -> Dict:
    out = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))) for k, v in b.items()
           if k in ("individual_features", "returns", "mask", "macro_features") and v is not None}
    return {k: v.detach().cpu() for k, v in out.items()}


def _fit_cpu(config, names, tb, fs, cs, epochs, lr, seeds, keep_models, dtype=torch.float32):
    from ..models.gan import AssetPricingGAN
    from ..engine.runner import flatten_state
    hists, best_ep, best_loss, preds, models, finals = [], [], [], {s: [] for s in names}, [], []
    ft = {s: None if fs[s] is None else torch.from_numpy(fs[s]).to(dtype) for s in names}
    ct = {s: torch.from_numpy(cs[s]).to(dtype) for s in names}
    for seed in seeds:
        torch.manual_seed(int(seed))
        model = AssetPricingGAN(config).to(dtype)
        params = list(model.sdf_net.parameters())
        opt = torch.optim.Adam(params, lr=lr)
        hist = np.full((epochs, len(HIST)), np.nan, dtype=np.float64 if dtype == torch.float64 else np.float32)
        best, bep, snap = float("inf"), -1, None
        for ep in range(epochs):
            model.train()
            opt.zero_grad()
            loss = _torch_loss(_raw_output(model, tb["train"], dtype), tb["train"], ft["train"], ct["train"])
            loss.backward()
            gn = torch.nn.utils.clip_grad_norm_(params, max_norm=GRAD_CLIP)
            opt.step()
            model.eval()
            row = [loss.item(), np.nan, np.nan, float(gn), 0.0]
            with torch.no_grad():
                for s in names[1:]:
                    row[HIST[s + "_loss"]] = float(_torch_loss(_raw_output(model, tb[s], dtype), tb[s], ft[s], ct[s]))
            v = np.float32(row[HIST["valid_loss"]])
            if v < best:                                   # (NaN never wins)
                best, bep, snap = float(v), ep, copy.deepcopy(model.state_dict())
                row[HIST["best"]] = 1.0
            hist[ep] = row
        if keep_models:
            finals.append(flatten_state(model, model.spec))
        if snap is not None:
            model.load_state_dict(snap)
        model.eval()
        with torch.no_grad():
            for s in names:
                p = _raw_output(model, tb[s], dtype).numpy().astype(np.float64)
                preds[s].append(np.where(tb[s]["mask"].bool().numpy(), p, 0.0))
        hists.append(hist); best_ep.append(bep); best_loss.append(best)
        if keep_models:
            models.append(model)
    return hists, best_ep, best_loss, preds, models, finals


def _fit_gpu(config, names, tb, fs, epochs, lr, seeds, weighting, precision, keep_models):
    from ..engine.runner import GANEngine
    from ..models.gan import AssetPricingGAN
    G = len(seeds)
    models = []
    for seed in seeds:
        torch.manual_seed(int(seed))
        models.append(AssetPricingGAN(config))
    eng = GANEngine(models[0].spec, G, max_epochs=max(epochs, 1), precision=precision)
    eng.set_data(*[tb.get(s) for s in SPLITS])
    for g, (m, seed) in enumerate(zip(models, seeds)):
        eng.set_model(g, m, int(seed))
    e = eng.eng
    e.fit_begin([fs.get(s) for s in SPLITS], weighting)
    e.fit_epochs(int(epochs), float(lr))
    e.sync()
    if e.prog_timeouts():
        raise RuntimeError("fused LSTM + tower forward: a spin wait gave up, so the fit stopped updating "
                           "(the GPU is shared with other processes?); rerun with DLAP_RNN_OVERLAP=0")
    hists = [np.asarray(e.fit_history(g)) for g in range(G)]
    bests = [e.fit_best(g) for g in range(G)]
    finals = [np.asarray(e.get_params(g)) for g in range(G)] if keep_models else []
    e.fit_load_best()
    preds = {s: [] for s in names}
    for s in names:
        si = SPLITS.index(s)
        T, N = tb[s]["mask"].shape
        e.forward_split(si, False, False)
        rowti = eng.splits[si].rowti
        for g in range(G):
            w = np.asarray(e.read_ws(g, si, "w"))[:eng.splits[si].R]
            p = np.zeros((T, N))
            p[rowti[:, 0], rowti[:, 1]] = w
            preds[s].append(p)
    out_models = []
    if keep_models:
        for g, m in enumerate(models):
            m.load_state_dict(eng.state_dict(g))
            out_models.append(m)
    return hists, [int(b[0]) for b in bests], [float(b[1]) for b in bests], preds, out_models, finals


def fit_prediction(config: Dict, batches: Dict[str, Dict], factor: Optional[Dict] = None, device: str = "cpu",
                   epochs: int = 64, lr: Optional[float] = None, seeds: Sequence[int] = (0,),
                   weighting: str = "period", precision: str = "bf16", keep_models: bool = False,
                   cpu_dtype: torch.dtype = torch.float32) -> Dict:
    """Fit ``len(seeds)`` towers of ``AssetPricingGAN(config).sdf_net``'s architecture to
    ``y = R f`` on ``batches["train"]``, selecting each at its best epoch on ``batches["valid"]``.

    ``factor``: ``{split: [T] float32}`` or None (ones). ``lr`` defaults to the config's
    ``learning_rate`` (1e-3). Returns ``prediction`` (by split: the dense [T][N] float64 mean over
    the seeds of the selected towers' raw outputs, 0 at the invalid entries), ``history`` (per seed
    [epochs][5]: train, valid, test loss, gradient norm, is_best), ``best_epoch``, ``best_loss``,
    ``loss_zero`` (by split: the zero predictor's loss), ``device`` and, with ``keep_models``,
    ``models`` (the selected towers) and ``final_params`` (per seed: the flat parameter vector after
    the last epoch, before the selection). ``cpu_dtype=torch.float64`` runs the torch loop in double
    precision (the reference the fp32 executors are measured against; its history rows are float64)."""
    names = _names(batches)
    if weighting not in ("period", "pooled"):
        raise ValueError("weighting must be 'period' or 'pooled'")
    epochs = int(epochs)
    if epochs < 1 or len(seeds) < 1:
        raise ValueError("fit_prediction needs at least one epoch and one seed")
    lr = float(config.get("learning_rate", 1e-3) if lr is None else lr)
    tb = {s: _tensor_batch(batches[s]) for s in names}
    fs = {s: _factor_of(factor, s, int(tb[s]["mask"].shape[0])) for s in names}
    cs = {s: row_weights(tb[s]["mask"], weighting) for s in names}
    use_gpu = False
    if str(device).startswith("cuda"):
        from ..ops import native
        if native.load(required=False) is None:
            print("[prediction] native extension not available: using the CPU path")
        else:
            use_gpu = True
    if use_gpu:
        hists, bep, bl, preds, models, finals = _fit_gpu(config, names, tb, fs, epochs, lr, list(seeds), weighting,
                                                         precision, keep_models)
    else:
        hists, bep, bl, preds, models, finals = _fit_cpu(config, names, tb, fs, cs, epochs, lr, list(seeds), keep_models,
                                                         cpu_dtype)
    out = {"prediction": {s: np.mean(np.stack(preds[s]), axis=0) for s in names}, "history": hists,
           "best_epoch": bep, "best_loss": bl, "device": "cuda" if use_gpu else "cpu", "weighting": weighting,
           "epochs": epochs, "lr": lr, "seeds": [int(s) for s in seeds]}
    out["loss_zero"] = {}
    for s in names:
        z = np.zeros(tb[s]["mask"].shape, np.float32)
        out["loss_zero"][s] = prediction_sums_numpy(z, tb[s]["returns"], tb[s]["mask"], fs[s], weighting)["loss_zero"]
    if keep_models:
        out["models"], out["final_params"] = models, finals
    return out


# ---------------------------------------------------------------------------------------------
# The two users

def ffn_benchmark(batches: Dict[str, Dict], config: Dict, device: str = "cpu", epochs: int = 64,
                  lr: Optional[float] = None, seeds: Sequence[int] = (0,), weighting: str = "period",
                  precision: str = "bf16") -> Dict:
    """The FFN return-prediction benchmark: ``f = 1``, SDF weights ``omega`` = the prediction,
    L1-normalised per period (``portfolio.renormalize``), natural sign ``+omega.R`` as for LS / EN.

    Returns a row in the shape of ``benchmarks.linear_benchmarks``'s: ``sharpe``, ``ev``, ``xs_r2``,
    ``r2`` (the prediction R²), ``factor`` and ``weights`` by split, plus ``history``,
    ``best_epoch``, ``best_loss``, ``loss_zero`` and ``device``."""
    fit = fit_prediction(config, batches, None, device, epochs, lr, seeds, weighting, precision)
    row = {"sharpe": {}, "ev": {}, "xs_r2": {}, "r2": {}, "factor": {}, "weights": {}}
    for s, p in fit["prediction"].items():
        r, m = _np(batches[s]["returns"], np.float64), _np(batches[s]["mask"]).astype(bool)
        w = renormalize(p, m)
        f = (w * r * m).sum(axis=1)
        sy = float((r * r * m).sum())
        row["weights"][s], row["factor"][s] = w, f
        row["sharpe"][s] = sharpe_ddof0(f)
        row["ev"][s] = explained_variation(w, r, m)
        row["xs_r2"][s] = cross_sectional_r2(w, r, m)
        row["r2"][s] = 1.0 - float((((p - r) * m) ** 2).sum()) / sy if sy > 0 else float("nan")
    row.update({k: fit[k] for k in ("history", "best_epoch", "best_loss", "loss_zero", "device", "epochs", "lr", "seeds")})
    return row


def sdf_factor(weights, returns, mask) -> np.ndarray:
    """``f[t] = sum_i w[t,i] R[t,i]`` over the valid entries, float32 (the beta network's target scale)."""
    w, r, m = _np(weights, np.float64), _np(returns, np.float64), _np(mask).astype(bool)
    return (w * r * m).sum(axis=1).astype(np.float32)


def beta_network(weights_by_split: Dict[str, np.ndarray], batches: Dict[str, Dict], config: Dict,
                 device: str = "cpu", epochs: int = 64, lr: Optional[float] = None, seeds: Sequence[int] = (0,),
                 weighting: str = "period", precision: str = "bf16") -> Dict:
    """The beta network: a tower fitted to ``R[t,i] F[t]`` with ``F[t] = sum_i w[t,i] R[t,i]`` from the
    given (ensemble) weights of each split, fitted on train and selected on valid.

    EV and XS-R² are invariant to the sign and per-period scale of the loadings, so ``F`` is given
    the sign that makes its train mean non-negative: flipping the sign of the input weights
    changes nothing. Returns ``beta`` (by split: [T][N] float64), ``ev`` and ``xs_r2`` (by split:
    ``portfolio.explained_variation`` / ``cross_sectional_r2`` with loadings ``beta``), ``factor``
    (the targets' ``F``), ``history``, ``best_epoch``, ``best_loss``, ``loss_zero`` and ``device``."""
    names = _names(batches)
    fs = {s: sdf_factor(weights_by_split[s], batches[s]["returns"], batches[s]["mask"]) for s in names}
    if float(fs["train"].astype(np.float64).sum()) < 0.0:
        fs = {s: -f for s, f in fs.items()}
    fit = fit_prediction(config, batches, fs, device, epochs, lr, seeds, weighting, precision)
    out = {"beta": fit["prediction"], "factor": fs, "ev": {}, "xs_r2": {}}
    for s, b in fit["prediction"].items():
        r, m = _np(batches[s]["returns"], np.float64), _np(batches[s]["mask"]).astype(bool)
        out["ev"][s] = explained_variation(b, r, m)
        out["xs_r2"][s] = cross_sectional_r2(b, r, m)
    out.update({k: fit[k] for k in ("history", "best_epoch", "best_loss", "loss_zero", "device", "epochs", "lr", "seeds")})
    return out


# ---------------------------------------------------------------------------------------------
# Printing / JSON

def format_ffn_row(row: Dict) -> str:
    """The FFN line of the benchmark table (``benchmarks.format_benchmarks``'s columns)."""
    g = lambda d, s: d.get(s, float("nan"))
    return (f"  {'FFN':14s} {g(row['sharpe'], 'train'):9.4f} {g(row['sharpe'], 'valid'):9.4f} {g(row['sharpe'], 'test'):9.4f} "
            f"{g(row['ev'], 'test'):9.4f} {g(row['xs_r2'], 'test'):11.4f}")


def format_beta(res: Dict, proxy: Optional[Dict] = None) -> List[str]:
    """Per split: EV / XS-R² with the beta network's loadings, next to the proxy figures (the SDF
    weight vector as the loading direction: ``proxy[split] = {"ev", "xs_r2"}``) when given."""
    lines = []
    for s in SPLITS:
        if s not in res["ev"]:
            continue
        line = f"  {s.capitalize():5s}  EV (beta net) {res['ev'][s]:7.4f}  XS-R2 (beta net) {res['xs_r2'][s]:7.4f}"
        if proxy is not None and s in proxy:
            line += f"  |  EV (proxy) {proxy[s]['ev']:7.4f}  XS-R2 (proxy) {proxy[s]['xs_r2']:7.4f}"
        lines.append(line)
    lines.append(f"  beta net: {len(res['seeds'])} seed(s), {res['epochs']} epochs, lr {res['lr']:.3g}, best epoch(s) "
                 f"{[int(e) + 1 for e in res['best_epoch']]}, device {res['device']}")
    return lines


def to_json(res: Dict) -> Dict:
    """Plain lists of an ``ffn_benchmark`` / ``beta_network`` result without its dense arrays."""
    from .benchmarks import _jsonable
    return _jsonable({k: v for k, v in res.items() if k not in ("weights", "beta", "models")})

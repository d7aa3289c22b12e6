"""Raw characteristic panels: the cross-sectional rank transform and ``src.prepare_data``.

The model, the knock-outs and the sorted portfolios assume the paper's panel: every
characteristic rank-normalised into (-0.5, 0.5) within its month, and a stock-month present only
if all of its characteristics are. This module turns a raw panel (levels, heavy tails, single
missing entries) into that form; the result is an ordinary ``data_dir``.

Definition (``rank_characteristics_numpy``, the oracle of ``csrc/k_xrank.hip``). With
``thr = float32(MISSING_VALUE + 1)``, element ``(t, i, f)`` participates iff ``rowok[t, i]`` and
``x[t, i, f] > thr`` (a NaN compares false and is missing, ``+inf`` participates). Per ``(t, f)``
over the participants ``A``, ``m = |A|`` (``cnt[t, f]``) and for ``i`` in ``A``::

    lt = #{j in A: x_j < x_i},  eq = #{j in A: x_j == x_i}     (IEEE: -0 == +0, eq counts i)
    y[t, i, f] = float32(2 lt + eq - m) / float32(2 m)           (one fp32 division)

the average-tie rank ``r = lt + (eq + 1) / 2`` mapped by ``(r - 0.5) / m - 0.5``: antisymmetric,
the numerators of a column sum to 0, the median is 0. A missing element of a kept row becomes
``fill_missing`` (0, the column's median), a row that is not kept ``fill_dead``.

Factor imputation (``impute="xs"``; the cross-sectional model of Bryzgalova, Lettau, Lerner and
Pelger, "Missing Financial Data"). On the ranked panel ``y`` (holes NaN), element ``(t, i, f)`` is
observed, ``o = 1``, iff ``rowok[t, i]`` and ``y == y``; ``z = y`` where observed, else 0 (dead rows
and holes may hold anything: they are selected, never multiplied). Per period::

    S[a][b] = sum_i z_ia z_ib (float64),  C[a][b] = sum_i o_ia o_ib     characteristic_moments_numpy
    Sig = S / C (0 where C = 0);  lam = the K' = min(K, F) top eigenvectors of Sig, descending,
          each signed so that its largest-magnitude component is positive, float32     xs_loadings
    A = gamma I + sum_{f observed} lam_f lam_f',  b = sum_{f observed} lam_f y_f,  g = A^-1 b
    out[t, i, f] = float32(clip(lam_f . g, -0.5, 0.5)) for every f not observed      xs_fill_numpy

Observed entries and dead rows keep their bits. ``csrc/k_ximpute.hip`` holds the GPU kernels
(``k_ximp_gram``, ``k_ximp_fill``); the eigenproblem is host numpy float64 on every path.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import time
from typing import Optional, Sequence

import numpy as np
import torch

from .dataset import MISSING_VALUE, _npz_member

THR = np.float32(MISSING_VALUE + 1)            # the loader's threshold
IMPUTE = ("none", "median", "xs")


def rank_characteristics_numpy(x, rowok, fill_missing: float = 0.0, fill_dead: float = MISSING_VALUE):
    """The definition: ``x`` float32 [T][N][F], ``rowok`` bool [T][N] -> (``y`` float32 [T][N][F],
    ``cnt`` int32 [T][F])."""
    x = np.asarray(x, dtype=np.float32)
    rowok = np.asarray(rowok, dtype=bool)
    T, N, F = x.shape
    y = np.empty((T, N, F), dtype=np.float32)
    cnt = np.zeros((T, F), dtype=np.int32)
    for t in range(T):
        ok = rowok[t]
        base = np.where(ok, np.float32(fill_missing), np.float32(fill_dead)).astype(np.float32)
        for f in range(F):
            col = x[t, :, f]
            part = ok & (col > THR)
            m = int(part.sum())
            cnt[t, f] = m
            out = base.copy()
            if m:
                v = col[part]
                s = np.sort(v)
                lt = np.searchsorted(s, v, side="left")
                le = np.searchsorted(s, v, side="right")          # lt + eq
                out[part] = (lt + le - m).astype(np.float32) / np.float32(2 * m)
            y[t, :, f] = out
    return y, cnt


def row_filter(ret, x, impute: str = "none", min_characteristics: int = 1):
    """The rows a prepared panel keeps: a return, and every characteristic (``impute="none"``, the
    reference's rule) or at least ``max(1, min_characteristics)`` of them (``"median"``, ``"xs"``)."""
    if impute not in IMPUTE:
        raise ValueError(f"impute must be one of {IMPUTE}, got {impute!r}")
    ret = np.asarray(ret)
    x = np.asarray(x)
    ret_ok = (ret > THR) & ~np.isnan(ret)
    present = (x > THR).sum(axis=-1)
    if impute == "none":
        return ret_ok & (present == x.shape[-1])
    return ret_ok & (present >= max(1, int(min_characteristics)))


def _resolve_device(device) -> Optional[torch.device]:
    """None: the numpy path. ``None`` / ``"auto"`` pick the current GPU when there is one."""
    if device is None or device == "auto":
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    dev = torch.device(device)
    if dev.type == "cpu":
        return None
    if dev.type != "cuda":
        raise ValueError(f"device must be auto, cpu or cuda[:k], got {device!r}")
    if not torch.cuda.is_available():
        raise RuntimeError(f"device {device!r} requested but no GPU is available")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _rank_device(nat, x: torch.Tensor, ok: torch.Tensor, out: torch.Tensor, cnt: torch.Tensor,
                 fill_missing: float, fill_dead: float) -> None:
    T, N, F = x.shape
    with torch.cuda.device(x.device):
        nat.rank_characteristics(x.data_ptr(), ok.data_ptr(), out.data_ptr(), cnt.data_ptr(), T, N, F, float(THR),
                                 float(fill_missing), float(fill_dead), torch.cuda.current_stream(x.device).cuda_stream)


def _note_unsupported(N: int, nat) -> None:
    print(f"[rank_characteristics] N = {N} is above XRANK_MAX_N = {nat.XRANK_MAX_N}: using the numpy path")


def rank_characteristics(x, rowok, *, device=None, out=None, chunk_bytes: int = 1 << 30,
                         fill_missing: float = 0.0, fill_dead: float = MISSING_VALUE):
    """Rank transform of ``x`` [T][N][F] over the rows ``rowok`` [T][N] -> ``(y, cnt)``.

    A CUDA tensor (float32, contiguous) is ranked where it lies by ``k_xrank``; ``out=x`` ranks in
    place without a copy. A host array goes up in period chunks of at most ``chunk_bytes``, is
    ranked in place on the device and comes back (``out`` may be ``x`` or any float32 array of its
    shape). ``device="cpu"``, or a machine without a GPU, runs the numpy definition. With a GPU
    the native extension has to load: there is no eager fallback.
    """
    if isinstance(x, torch.Tensor) and x.is_cuda:
        from ..ops import native
        nat = native.load(required=True)
        if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 3:
            raise ValueError("a device panel must be a contiguous float32 [T][N][F] tensor")
        T, N, F = x.shape
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError("out must match x (shape, float32, device, contiguous)")
        ok = torch.as_tensor(rowok).to(x.device, torch.uint8).contiguous()
        if tuple(ok.shape) != (T, N):
            raise ValueError("rowok must be [T][N]")
        if not nat.rank_supported(N):
            _note_unsupported(N, nat)
            y, c = rank_characteristics_numpy(x.cpu().numpy(), ok.cpu().numpy().astype(bool), fill_missing, fill_dead)
            out.copy_(torch.from_numpy(y))
            return out, torch.from_numpy(c).to(x.device)
        cnt = torch.empty((T, F), dtype=torch.int32, device=x.device)
        if T:
            _rank_device(nat, x, ok, out, cnt, fill_missing, fill_dead)
        return out, cnt

    x = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    rowok = np.asarray(rowok.cpu().numpy() if isinstance(rowok, torch.Tensor) else rowok, dtype=bool)
    if x.ndim != 3 or rowok.shape != x.shape[:2]:
        raise ValueError("x must be [T][N][F] and rowok [T][N]")
    T, N, F = x.shape
    dev = _resolve_device(device)
    nat = None
    if dev is not None:
        from ..ops import native
        nat = native.load(required=True)
        if not nat.rank_supported(N):
            _note_unsupported(N, nat)
            dev = None
    if dev is None:
        y, cnt = rank_characteristics_numpy(x, rowok, fill_missing, fill_dead)
        if out is None:
            return y, cnt
        out[...] = y
        return out, cnt
    if out is None:
        out = np.empty((T, N, F), dtype=np.float32)
    cnt = np.empty((T, F), dtype=np.int32)
    step = max(1, int(chunk_bytes) // max(1, N * F * 4))
    for t0 in range(0, T, step):                       # one chunk resident: up, ranked in place, back
        t1 = min(T, t0 + step)
        xd = torch.from_numpy(np.ascontiguousarray(x[t0:t1], dtype=np.float32)).to(dev)
        okd = torch.from_numpy(rowok[t0:t1].astype(np.uint8)).to(dev)
        cd = torch.empty((t1 - t0, F), dtype=torch.int32, device=dev)
        _rank_device(nat, xd, okd, xd, cd, fill_missing, fill_dead)
        out[t0:t1] = xd.cpu().numpy()
        cnt[t0:t1] = cd.cpu().numpy()
        del xd, okd, cd
    return out, cnt


# ---- factor imputation (the "xs" model) -----------------------------------------------------------
def _observed(y, rowok):
    return rowok[..., None] & (y == y)


def characteristic_moments_numpy(y, rowok):
    """The definition: ``y`` float32 [T][N][F] (NaN marks a hole), ``rowok`` [T][N] ->
    (``S`` float64 [T][F][F], ``C`` int32 [T][F][F]) over the observed entries."""
    y = np.asarray(y, dtype=np.float32)
    rowok = np.asarray(rowok, dtype=bool)
    T, N, F = y.shape
    S = np.zeros((T, F, F), dtype=np.float64)
    C = np.zeros((T, F, F), dtype=np.int32)
    for t in range(T):
        o = _observed(y[t], rowok[t])
        z = np.where(o, y[t], np.float32(0)).astype(np.float64)       # selected, never multiplied
        oi = o.astype(np.int32)
        S[t] = z.T @ z
        C[t] = oi.T @ oi
    return S, C


def xs_loadings(S, C, K: int):
    """``S``, ``C`` [T][F][F] -> (``lam`` float32 [T][F][K'], ``explained`` float64 [T]),
    ``K' = min(K, F)``. Host numpy float64 on every path."""
    S = np.asarray(S, dtype=np.float64)
    C = np.asarray(C)
    T, F, _ = S.shape
    if int(K) < 1:
        raise ValueError(f"K must be at least 1, got {K}")
    Kp = min(int(K), F)
    lam = np.zeros((T, F, Kp), dtype=np.float32)
    explained = np.zeros(T, dtype=np.float64)
    for t in range(T):
        if not (C[t] > 0).any():                       # a period without a kept row
            continue
        sig = np.where(C[t] > 0, S[t] / np.maximum(C[t], 1), 0.0)
        w, V = np.linalg.eigh(sig)
        top = np.argsort(w, kind="stable")[::-1][:Kp]
        v = V[:, top]
        big = np.abs(v).argmax(axis=0)                 # (the first such component on a tie)
        v = v * np.where(v[big, np.arange(Kp)] < 0, -1.0, 1.0)
        lam[t] = v.astype(np.float32)
        pos = np.maximum(w, 0.0)
        den = pos.sum()
        explained[t] = pos[top].sum() / den if den > 0 else 0.0
    return lam, explained


def xs_fill_numpy(y, rowok, lam, gamma: float = 0.01, out=None):
    """The definition: the holes of every row with ``rowok`` become the clipped fitted values of the
    ridge regression of its observed entries on ``lam[t]`` (float64 from the float32 ``y`` and
    ``lam``); everything else keeps its bits. ``out`` may be ``y``."""
    if not gamma > 0:
        raise ValueError(f"gamma must be positive, got {gamma}")
    y = np.asarray(y, dtype=np.float32)
    rowok = np.asarray(rowok, dtype=bool)
    lam = np.asarray(lam, dtype=np.float32)
    T, N, F = y.shape
    if lam.ndim != 3 or lam.shape[:2] != (T, F) or rowok.shape != (T, N):
        raise ValueError("y must be [T][N][F], rowok [T][N] and lam [T][F][K]")
    Kp = lam.shape[2]
    if out is None:
        out = y.copy()
    elif out is not y:
        out[...] = y
    for t in range(T):
        rows = np.flatnonzero(rowok[t])
        if rows.size == 0:
            continue
        yt = y[t, rows]
        o = yt == yt
        if o.all():
            continue
        l64 = lam[t].astype(np.float64)
        z = np.where(o, yt, np.float32(0)).astype(np.float64)
        P = (l64[:, :, None] * l64[:, None, :]).reshape(F, Kp * Kp)
        A = (o.astype(np.float64) @ P).reshape(-1, Kp, Kp) + float(gamma) * np.eye(Kp)
        g = np.linalg.solve(A, (z @ l64)[:, :, None])[:, :, 0]
        fit = np.clip(g @ l64.T, -0.5, 0.5).astype(np.float32)
        out[t, rows] = np.where(o, yt, fit)
    return out


def _note_ximp(what: str, F: int, K: int) -> None:
    print(f"[{what}] F = {F}, K = {K} is outside ximp_supported: using the numpy path")


def _moments_device(nat, y: torch.Tensor, ok: torch.Tensor, S: torch.Tensor, C: torch.Tensor) -> None:
    T, N, F = y.shape
    with torch.cuda.device(y.device):
        nat.characteristic_moments(y.data_ptr(), ok.data_ptr(), S.data_ptr(), C.data_ptr(), T, N, F,
                                   torch.cuda.current_stream(y.device).cuda_stream)


def _fill_device(nat, y: torch.Tensor, ok: torch.Tensor, lam: torch.Tensor, out: torch.Tensor, gamma: float) -> None:
    T, N, F = y.shape
    with torch.cuda.device(y.device):
        nat.xs_fill(y.data_ptr(), ok.data_ptr(), lam.data_ptr(), out.data_ptr(), T, N, F, lam.shape[2], float(gamma),
                    torch.cuda.current_stream(y.device).cuda_stream)


def _check_device_panel(y: torch.Tensor, rowok):
    if y.dtype != torch.float32 or not y.is_contiguous() or y.dim() != 3:
        raise ValueError("a device panel must be a contiguous float32 [T][N][F] tensor")
    ok = rowok if isinstance(rowok, torch.Tensor) else torch.from_numpy(np.array(rowok, dtype=np.uint8))
    ok = ok.to(y.device, torch.uint8).contiguous()
    if tuple(ok.shape) != tuple(y.shape[:2]):
        raise ValueError("rowok must be [T][N]")
    return ok


def _host_panel(y, rowok):
    y = np.asarray(y.numpy() if isinstance(y, torch.Tensor) else y)
    rowok = np.asarray(rowok.cpu().numpy() if isinstance(rowok, torch.Tensor) else rowok, dtype=bool)
    if y.ndim != 3 or rowok.shape != y.shape[:2]:
        raise ValueError("y must be [T][N][F] and rowok [T][N]")
    return y, rowok


def characteristic_moments(y, rowok, *, device=None, chunk_bytes: int = 1 << 30):
    """Masked second moments of a ranked panel ``y`` [T][N][F] (holes NaN) -> ``(S, C)``.

    A CUDA tensor (float32, contiguous) is read where it lies by ``k_ximp_gram`` and ``S``, ``C``
    stay on its device. A host array goes up in period chunks of at most ``chunk_bytes`` and numpy
    arrays come back. ``device="cpu"``, or a machine without a GPU, runs the numpy definition. With
    a GPU the native extension has to load: there is no eager fallback."""
    if isinstance(y, torch.Tensor) and y.is_cuda:
        from ..ops import native
        nat = native.load(required=True)
        ok = _check_device_panel(y, rowok)
        T, N, F = y.shape
        if not nat.ximp_supported(F, 1) or N < 1:
            _note_ximp("characteristic_moments", F, 1)
            S, C = characteristic_moments_numpy(y.cpu().numpy(), ok.cpu().numpy().astype(bool))
            return torch.from_numpy(S).to(y.device), torch.from_numpy(C).to(y.device)
        S = torch.empty((T, F, F), dtype=torch.float64, device=y.device)
        C = torch.empty((T, F, F), dtype=torch.int32, device=y.device)
        if T:
            _moments_device(nat, y, ok, S, C)
        return S, C

    y, rowok = _host_panel(y, rowok)
    T, N, F = y.shape
    dev = _resolve_device(device)
    nat = None
    if dev is not None:
        from ..ops import native
        nat = native.load(required=True)
        if not nat.ximp_supported(F, 1) or N < 1:
            _note_ximp("characteristic_moments", F, 1)
            dev = None
    if dev is None:
        return characteristic_moments_numpy(y, rowok)
    S = np.empty((T, F, F), dtype=np.float64)
    C = np.empty((T, F, F), dtype=np.int32)
    step = max(1, int(chunk_bytes) // max(1, N * F * 4))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        yd = torch.from_numpy(np.ascontiguousarray(y[t0:t1], dtype=np.float32)).to(dev)
        okd = torch.from_numpy(rowok[t0:t1].astype(np.uint8)).to(dev)
        Sd = torch.empty((t1 - t0, F, F), dtype=torch.float64, device=dev)
        Cd = torch.empty((t1 - t0, F, F), dtype=torch.int32, device=dev)
        _moments_device(nat, yd, okd, Sd, Cd)
        S[t0:t1] = Sd.cpu().numpy()
        C[t0:t1] = Cd.cpu().numpy()
        del yd, okd, Sd, Cd
    return S, C


def xs_fill(y, rowok, lam, gamma: float = 0.01, *, out=None, device=None, chunk_bytes: int = 1 << 30):
    """Fill the holes of a ranked panel ``y`` [T][N][F] from the loadings ``lam`` [T][F][K'] -> ``out``.

    A CUDA tensor is filled where it lies by ``k_ximp_fill`` (``out=y``: in place, only the holes are
    written). A host array goes up in period chunks of at most ``chunk_bytes``. ``device="cpu"``, or
    a machine without a GPU, runs the numpy definition. With a GPU the native extension has to
    load: there is no eager fallback."""
    if not gamma > 0:
        raise ValueError(f"gamma must be positive, got {gamma}")
    if isinstance(y, torch.Tensor) and y.is_cuda:
        from ..ops import native
        nat = native.load(required=True)
        ok = _check_device_panel(y, rowok)
        T, N, F = y.shape
        if out is None:
            out = torch.empty_like(y)
        elif out.shape != y.shape or out.dtype != y.dtype or out.device != y.device or not out.is_contiguous():
            raise ValueError("out must match y (shape, float32, device, contiguous)")
        lamd = lam if isinstance(lam, torch.Tensor) else torch.from_numpy(np.array(lam, dtype=np.float32))
        lamd = lamd.to(y.device, torch.float32).contiguous()
        if lamd.dim() != 3 or tuple(lamd.shape[:2]) != (T, F):
            raise ValueError("lam must be [T][F][K]")
        Kp = lamd.shape[2]
        if not nat.ximp_supported(F, Kp) or N < 1:
            _note_ximp("xs_fill", F, Kp)
            res = xs_fill_numpy(y.cpu().numpy(), ok.cpu().numpy().astype(bool), lamd.cpu().numpy(), gamma)
            out.copy_(torch.from_numpy(res))
            return out
        if T:
            _fill_device(nat, y, ok, lamd, out, gamma)
        return out

    y, rowok = _host_panel(y, rowok)
    lam = np.ascontiguousarray(lam.cpu().numpy() if isinstance(lam, torch.Tensor) else lam, dtype=np.float32)
    T, N, F = y.shape
    if lam.ndim != 3 or lam.shape[:2] != (T, F):
        raise ValueError("lam must be [T][F][K]")
    Kp = lam.shape[2]
    dev = _resolve_device(device)
    nat = None
    if dev is not None:
        from ..ops import native
        nat = native.load(required=True)
        if not nat.ximp_supported(F, Kp) or N < 1:
            _note_ximp("xs_fill", F, Kp)
            dev = None
    if dev is None:
        return xs_fill_numpy(y, rowok, lam, gamma, out=out)
    if out is None:
        out = np.empty((T, N, F), dtype=np.float32)
    step = max(1, int(chunk_bytes) // max(1, N * F * 4))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        yd = torch.from_numpy(np.ascontiguousarray(y[t0:t1], dtype=np.float32)).to(dev)
        okd = torch.from_numpy(rowok[t0:t1].astype(np.uint8)).to(dev)
        ld = torch.from_numpy(lam[t0:t1]).to(dev)
        _fill_device(nat, yd, okd, ld, yd, gamma)
        out[t0:t1] = yd.cpu().numpy()
        del yd, okd, ld
    return out


def _prepare_xs(x, rowok, out, dev, chunk_bytes: int, K: int, gamma: float):
    """Rank with NaN holes, moments, loadings, fill: ``out`` [T][N][F] (a view is fine) -> (``cnt``,
    ``explained`` [T]). On the GPU every period chunk is uploaded once and stays resident from the
    rank to the fill; only S, C (down) and lam (up) cross in between."""
    T, N, F = x.shape
    Kp = min(int(K), F)
    nat = None
    if dev is not None:
        from ..ops import native
        nat = native.load(required=True)
    if nat is None or not nat.rank_supported(N) or not nat.ximp_supported(F, Kp):
        d = "cpu" if dev is None else dev                      # the staged calls, each with its own rule
        y, cnt = rank_characteristics(x, rowok, device=d, chunk_bytes=chunk_bytes, fill_missing=float("nan"),
                                      fill_dead=MISSING_VALUE)
        S, C = characteristic_moments(y, rowok, device=d, chunk_bytes=chunk_bytes)
        lam, explained = xs_loadings(S, C, K)
        out[...] = xs_fill(y, rowok, lam, gamma, out=y, device=d, chunk_bytes=chunk_bytes)
        return cnt, explained
    cnt = np.empty((T, F), dtype=np.int32)
    explained = np.zeros(T, dtype=np.float64)
    step = max(1, int(chunk_bytes) // max(1, N * F * 4))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        xd = torch.from_numpy(np.ascontiguousarray(x[t0:t1], dtype=np.float32)).to(dev)
        okd = torch.from_numpy(rowok[t0:t1].astype(np.uint8)).to(dev)
        cd = torch.empty((t1 - t0, F), dtype=torch.int32, device=dev)
        Sd = torch.empty((t1 - t0, F, F), dtype=torch.float64, device=dev)
        Cd = torch.empty((t1 - t0, F, F), dtype=torch.int32, device=dev)
        _rank_device(nat, xd, okd, xd, cd, float("nan"), MISSING_VALUE)
        _moments_device(nat, xd, okd, Sd, Cd)
        lam, explained[t0:t1] = xs_loadings(Sd.cpu().numpy(), Cd.cpu().numpy(), K)
        ld = torch.from_numpy(lam).to(dev)
        _fill_device(nat, xd, okd, ld, xd, gamma)
        out[t0:t1] = xd.cpu().numpy()
        cnt[t0:t1] = cd.cpu().numpy()
        del xd, okd, cd, Sd, Cd, ld
    return cnt, explained


def prepare_split(data, impute: str = "none", min_characteristics: int = 1, device=None,
                  chunk_bytes: int = 1 << 30, impute_factors: int = 6, impute_ridge: float = 0.01):
    """``data`` [T][N][1 + F] (column 0 the return) -> ``(data', report)``: kept rows are
    ``[ret, y...]``, every other row is ``MISSING_VALUE`` throughout, so the loader reproduces the
    kept rows as its mask and ``y`` as its features. ``impute="xs"`` fills the holes of the kept rows
    from ``impute_factors`` cross-sectional factors with the ridge ``impute_ridge``."""
    t_start = time.perf_counter()
    data = np.asarray(data)
    T, N, C = data.shape
    F = C - 1
    ret, x = data[:, :, 0], data[:, :, 1:]
    ret_ok = (ret > THR) & ~np.isnan(ret)
    rowok = row_filter(ret, x, impute, min_characteristics)
    out = np.full((T, N, C), np.float32(MISSING_VALUE), dtype=np.float32)
    dev = _resolve_device(device)
    explained = None
    if impute == "xs":
        if int(impute_factors) < 1 or not impute_ridge > 0:
            raise ValueError("impute_factors must be at least 1 and impute_ridge positive")
        cnt, explained = _prepare_xs(x, rowok, out[:, :, 1:], dev, chunk_bytes, int(impute_factors), float(impute_ridge))
    else:
        _, cnt = rank_characteristics(x, rowok, device="cpu" if dev is None else dev, out=out[:, :, 1:],
                                      chunk_bytes=chunk_bytes, fill_missing=0.0, fill_dead=MISSING_VALUE)
    out[:, :, 0][rowok] = ret[rowok]
    kept = int(rowok.sum())
    report = {
        "T": int(T), "N": int(N), "F": int(F),
        "rows_with_return": int(ret_ok.sum()),
        "complete_rows": int((ret_ok & ((x > THR).sum(axis=-1) == F)).sum()),
        "kept_rows": kept,
        "coverage": [float(c) / kept if kept else 0.0 for c in cnt.sum(axis=0, dtype=np.int64)],
        "impute": impute, "min_characteristics": int(min_characteristics),
        "device": "cpu" if dev is None else str(dev),
        "seconds": time.perf_counter() - t_start,
    }
    if impute == "xs":
        has = rowok.any(axis=1)
        report.update({
            "impute_factors": int(impute_factors), "impute_ridge": float(impute_ridge),
            "imputed_entries": int(kept * F - int(cnt.sum(dtype=np.int64))),
            "explained": float(explained[has].mean()) if has.any() else 0.0,
        })
    return out, report


def prepare_data_dir(input_dir: str, output_dir: str, impute: str = "none", min_characteristics: int = 1,
                     splits: Sequence[str] = ("train", "valid", "test"), device="auto",
                     chunk_bytes: int = 1 << 30, impute_factors: int = 6, impute_ridge: float = 0.01) -> dict:
    """Prepare ``input_dir`` (``char/Char_{split}.npz``, ``macro/macro_{split}.npz``) into the same
    layout under ``output_dir`` (``np.savez``, uncompressed: the loader maps it). ``date``,
    ``variable`` and any other member are carried over, macro files are copied byte for byte."""
    report = {}
    os.makedirs(os.path.join(output_dir, "char"), exist_ok=True)
    for s in splits:
        src = os.path.join(input_dir, "char", f"Char_{s}.npz")
        with np.load(src) as z:
            rest = {k: z[k] for k in z.files if k != "data"}
        data, rep = prepare_split(_npz_member(src, "data"), impute, min_characteristics, device, chunk_bytes,
                                  impute_factors, impute_ridge)
        np.savez(os.path.join(output_dir, "char", f"Char_{s}.npz"), data=data, **rest)
        mac = os.path.join(input_dir, "macro", f"macro_{s}.npz")
        if os.path.exists(mac):
            os.makedirs(os.path.join(output_dir, "macro"), exist_ok=True)
            shutil.copyfile(mac, os.path.join(output_dir, "macro", f"macro_{s}.npz"))
        report[s] = rep
    return report


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(prog="src.prepare_data",
                                 description="Rank-normalise a raw characteristic panel into a data_dir")
    ap.add_argument("--input_dir", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--impute", choices=IMPUTE, default="none")
    ap.add_argument("--impute_factors", type=int, default=6, help="xs: factors per period")
    ap.add_argument("--impute_ridge", type=float, default=0.01, help="xs: ridge of the per-row fit")
    ap.add_argument("--min_characteristics", type=int, default=1)
    ap.add_argument("--splits", nargs="+", default=["train", "valid", "test"])
    ap.add_argument("--device", default="auto", help="auto | cpu | cuda[:k]")
    ap.add_argument("--report", default=None, help="also write the report to this JSON file")
    a = ap.parse_args(argv)
    report = prepare_data_dir(a.input_dir, a.output_dir, a.impute, a.min_characteristics, a.splits, a.device,
                              impute_factors=a.impute_factors, impute_ridge=a.impute_ridge)
    for s, r in report.items():
        cov = r["coverage"]
        print(f"[prepare_data] {s}: T {r['T']} N {r['N']} F {r['F']}  rows with a return {r['rows_with_return']}  "
              f"complete {r['complete_rows']}  kept {r['kept_rows']}  coverage min {min(cov):.4f} mean "
              f"{sum(cov) / len(cov):.4f}  impute {r['impute']} (min {r['min_characteristics']})  "
              f"device {r['device']}  {r['seconds']:.3f} s")
        if r["impute"] == "xs":
            print(f"[prepare_data] {s}: xs  factors {r['impute_factors']}  ridge {r['impute_ridge']:g}  imputed entries "
                  f"{r['imputed_entries']}  explained {r['explained']:.4f}")
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main()

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
IMPUTE = ("none", "median")


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
    reference's rule) or at least ``max(1, min_characteristics)`` of them (``"median"``)."""
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


def prepare_split(data, impute: str = "none", min_characteristics: int = 1, device=None,
                  chunk_bytes: int = 1 << 30):
    """``data`` [T][N][1 + F] (column 0 the return) -> ``(data', report)``: kept rows are
    ``[ret, y...]``, every other row is ``MISSING_VALUE`` throughout, so the loader reproduces the
    kept rows as its mask and ``y`` as its features."""
    t_start = time.perf_counter()
    data = np.asarray(data)
    T, N, C = data.shape
    F = C - 1
    ret, x = data[:, :, 0], data[:, :, 1:]
    ret_ok = (ret > THR) & ~np.isnan(ret)
    rowok = row_filter(ret, x, impute, min_characteristics)
    out = np.full((T, N, C), np.float32(MISSING_VALUE), dtype=np.float32)
    dev = _resolve_device(device)
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
    return out, report


def prepare_data_dir(input_dir: str, output_dir: str, impute: str = "none", min_characteristics: int = 1,
                     splits: Sequence[str] = ("train", "valid", "test"), device="auto",
                     chunk_bytes: int = 1 << 30) -> dict:
    """Prepare ``input_dir`` (``char/Char_{split}.npz``, ``macro/macro_{split}.npz``) into the same
    layout under ``output_dir`` (``np.savez``, uncompressed: the loader maps it). ``date``,
    ``variable`` and any other member are carried over, macro files are copied byte for byte."""
    report = {}
    os.makedirs(os.path.join(output_dir, "char"), exist_ok=True)
    for s in splits:
        src = os.path.join(input_dir, "char", f"Char_{s}.npz")
        with np.load(src) as z:
            rest = {k: z[k] for k in z.files if k != "data"}
        data, rep = prepare_split(_npz_member(src, "data"), impute, min_characteristics, device, chunk_bytes)
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
    ap.add_argument("--min_characteristics", type=int, default=1)
    ap.add_argument("--splits", nargs="+", default=["train", "valid", "test"])
    ap.add_argument("--device", default="auto", help="auto | cpu | cuda[:k]")
    ap.add_argument("--report", default=None, help="also write the report to this JSON file")
    a = ap.parse_args(argv)
    report = prepare_data_dir(a.input_dir, a.output_dir, a.impute, a.min_characteristics, a.splits, a.device)
    for s, r in report.items():
        cov = r["coverage"]
        print(f"[prepare_data] {s}: T {r['T']} N {r['N']} F {r['F']}  rows with a return {r['rows_with_return']}  "
              f"complete {r['complete_rows']}  kept {r['kept_rows']}  coverage min {min(cov):.4f} mean "
              f"{sum(cov) / len(cov):.4f}  impute {r['impute']} (min {r['min_characteristics']})  "
              f"device {r['device']}  {r['seconds']:.3f} s")
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main()

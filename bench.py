"""Flagship benchmark: epochs/sec of the 3-phase GAN (BASELINE.json config 2) and the wall-clock of
the 9-model ensemble (config 3) on the N GPUs of one node.

Config: real-sized synthetic panel, T = 600 months split 240 / 60 / 300 (train / valid / test,
the paper's split), N = 3000 stocks, F = 46 characteristics, M = 178 macro series; the paper
architecture (LSTM [4] macro encoder, SDF FFN [64, 64], 8 tanh moments, dropout 0.05),
random init, bf16 tower GEMMs with fp32 accumulation / master weights / losses.

Metric: one timed "step" = one training epoch of the 3-phase schedule, drawn in the reference's
256 : 64 : 1024 proportion (phase 1 and 3 epochs include the valid + test evaluation, as in
`/root/reference/src/train.py:238-394`). Each rank (one per GPU) trains ``--models-per-gpu``
independently seeded models batched through the native engine; the reported value is the
whole-job aggregate model-epochs per second (weak scaling: fixed work per GPU), timed between
barriers + device synchronisations, max over ranks.

A plain run sets up, warms up, times the ``--steps`` epochs, writes ``--dump-outputs`` and prints
the result line; everything else the benchmark measures runs only with ``--full``.

Ensemble (``--full``; ``ensemble9`` in the output line, measured end to end, not extrapolated): the
real driver path `parallel.ensemble.run_ensemble` -- rank 0 generates the panel and RCCL-broadcasts
it, seeds 0..8 are sharded over the ranks and batched per rank into one engine (engine build,
panel compaction, hipGraph capture, the full 256 / 64 / 1024 schedule, final evaluation), the
best-Sharpe weights are all-gathered and the ensemble Sharpe is computed. The reference trains
the 9 seeds serially (`/root/reference/notebooks/demo_full.ipynb:1217-1246`).

Launch (the driver's two forms are equivalent):
    python bench.py --gpus N [--steps K --warmup W]          # spawns N ranks itself
    python bench.py --gpus N --full                          # ... plus the 9-model ensemble
    python bench.py --gpus 1 --dump-outputs DIR              # ... plus DIR/<name>.npy of the last step
    torchrun --nproc-per-node N bench.py --gpus N ...        # one rank per GPU from the env
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BENCH = dict(T_train=240, T_valid=60, T_test=300, N=3000, F=46, M=178)
# BASELINE config 5: the scaled panel (T=600, N=30000, F=512) through the wide layer-0 path
SCALED = dict(T_train=240, T_valid=60, T_test=300, N=30000, F=512, M=178)
# reference CPU epochs/sec on this exact config and schedule mix (tools/ref_baseline.py,
# 8-core Xeon, torch 2.10 CPU; see BASELINE.md "Measured on this box")
REF_EPOCHS_PER_S = float(os.environ.get("DLAP_REF_EPOCHS_PER_S", "0.397"))
# scaled panel: BASELINE.md measures the reference at a T=60 slice of 30000x512 (conditional step
# 6.0 s, evaluate 2.9 s); linear in rows, a 240/60/300 epoch is ~24 + 2.9 + 14.5 s -> ~0.025/s
REF_EPOCHS_PER_S_SCALED = 0.025
ENSEMBLE_SEEDS = tuple(range(9))           # BASELINE config 3: seeds 0-8


def make_panel(seed: int = 0, device: str = "cpu", T=None, N=None, F=None, M=None, cfg=None,
               keep_on_device: bool = False):
    """Synthetic panel split 240/60/300 with the reference's macro standardisation.
    ``keep_on_device``: leave the tensors on ``device`` (the engine then compacts the panel on
    the GPU; the scaled panel is 37 GB in fp32)."""
    from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
    cfg = cfg or BENCH
    Tt, Tv, Te = cfg["T_train"], cfg["T_valid"], cfg["T_test"]
    T = T or Tt + Tv + Te
    N, F, M = N or cfg["N"], F or cfg["F"], M or cfg["M"]
    ret, feats, mask, mac = generate_panel_fast(T, N, F, M, seed=seed, device=device)
    if not keep_on_device:
        ret, feats, mask, mac = ret.cpu(), feats.cpu(), mask.cpu(), mac.cpu()
    mu = mac[:Tt].mean(0, keepdim=True)
    sd = mac[:Tt].std(0, unbiased=False, keepdim=True) + 1e-8
    mac = (mac - mu) / sd
    cuts = [(0, Tt), (Tt, Tt + Tv), (Tt + Tv, T)]
    return tuple({"returns": ret[a:b].contiguous(), "individual_features": feats[a:b].contiguous(),
                  "mask": mask[a:b].contiguous(), "macro_features": mac[a:b].contiguous()} for a, b in cuts)


def schedule_split(k: int):
    """Split k epochs into the 256:64:1024 phase proportion (each >= 1 when k >= 3; the sum is
    always k: one or two epochs go to phase 3, then phase 1)."""
    if k < 3:
        return max(0, k - 1), 0, min(max(k, 0), 1)
    n1 = max(1, round(k * 256 / 1344))
    n2 = max(1, round(k * 64 / 1344))
    n3 = max(1, k - n1 - n2)
    return n1, n2, n3


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def visible_gpus() -> int:
    """GPUs the ranks will see, counted without touching HIP (no torch.cuda call in the parent):
    the KFD topology's GPU nodes (simd_count > 0), narrowed by the *_VISIBLE_DEVICES masks."""
    import glob
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:                        # no KFD sysfs (container without it): amdsmi's count,
        return torch.cuda.device_count()  # which does not initialise HIP on this image
    n = 0
    for f in nodes:
        try:
            with open(f) as fh:
                props = dict(line.split()[:2] for line in fh if len(line.split()) >= 2)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) > 0:
            n += 1
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def spawn_ranks(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N child ranks (one per GPU) with
    torchrun-style env and wait for them. The parent never touches the GPU (it counts devices from
    sysfs, ``visible_gpus``), so the children own their devices. Returns the exit code."""
    share = os.environ.get("DLAP_SHARE_GPU", "0") == "1"
    ndev = visible_gpus()
    if ndev < n and not share:
        print(f"bench.py: --gpus {n} requested but only {ndev} GPU(s) are visible", file=sys.stderr)
        return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0:
                    rc = rc or code
                    for q in pending:          # a dead rank would leave its peers in a collective
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def measure_ensemble(d, cfg, pc, seed_panel: int = 0):
    """End-to-end wall-clock of the 9-seed ensemble over the process group ``d`` (see module
    docstring). Returns the record for the output line (identical on all ranks)."""
    from deeplearninginassetpricing_paperreplication_amd.parallel import comm
    from deeplearninginassetpricing_paperreplication_amd.parallel.ensemble import run_ensemble
    comm.barrier(d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # the synthetic panel is generated on every rank's GPU from the same seed (bit-exact: the
    # same kernels and generator stream), so no rank waits for a broadcast; one small all-gather
    # of per-split checksums proves the copies identical (comm.broadcast_batches is the path for
    # panels read from disk, parallel/ensemble.py)
    tr, va, te = make_panel(seed=seed_panel, device=f"cuda:{d.local_rank}", cfg=pc, keep_on_device=True)
    batches = {"train": tr, "valid": va, "test": te}
    if d.active:
        ck = np.array([[float(torch.nan_to_num(b[k].double()).sum()) for b in (tr, va, te)
                        for k in ("returns", "individual_features")]])
        allck = comm.all_gather_rows(d, ck, d.world, [d.rank])
        if not (allck == allck[0:1]).all():
            raise RuntimeError("bench.py: ranks generated different synthetic panels")
    t_panel = time.perf_counter() - t0
    res = run_ensemble(cfg, batches, ENSEMBLE_SEEDS, d, epochs=(256, 64, 1024), lr=1e-3, ignore_epoch=64,
                       print_freq=1024)
    torch.cuda.synchronize()
    comm.barrier(d)
    wall = time.perf_counter() - t0
    if d.active:
        wall = max(comm.all_gather_rows(d, np.array([[wall]]), d.world, [d.rank])[:, 0])
    return {
        "wall_s": round(float(wall), 3), "measured": "end-to-end",
        "panel_setup_s_rank0": round(t_panel, 3),
        "train_wall_s_per_rank": [round(x, 3) for x in res["train_wall_s_per_rank"]],
        "models_per_rank": [len(comm.shard(len(ENSEMBLE_SEEDS), r, d.world)) for r in range(d.world)],
        "breakdown_s_per_rank": res.get("breakdown_s_per_rank"),
        "schedule": [256, 64, 1024], "seeds": list(ENSEMBLE_SEEDS), "failed": res["failed"],
        "test_sharpe": res.get("test_sharpe"), "valid_sharpe": res.get("valid_sharpe"),
        "reference_cpu_estimate_s": round(9 * 1344 / REF_EPOCHS_PER_S, 1),
    }


def dump_outputs(out_dir: str, eng, n_models: int, steps: int):
    """``--dump-outputs``: what a caller of the timed path holds after its last step, as float32
    ``<name>.npy``: ``params`` [G, P] (every model's flat parameters after the last Adam update),
    ``history_train`` [G, steps, columns] (the timed epochs' phase, train losses, train Sharpe,
    gradient norm and best-so-far trackers) and ``history_eval`` [G, phase-1 and phase-3 steps,
    columns] (their valid / test losses, Sharpe ratios and return statistics; phase 2 runs no
    evaluation). Columns in the order of ``engine.runner.HIST``; every stored element is one the
    run computed, so a NaN in a dump is a NaN of the run."""
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import HIST
    os.makedirs(out_dir, exist_ok=True)
    params = np.stack([np.asarray(eng.params(g), dtype=np.float32) for g in range(n_models)])
    hist = np.stack([np.asarray(eng.history_rows(g), dtype=np.float32)[-steps:] for g in range(n_models)])
    ev = sorted(c for k, c in HIST.items() if k.startswith(("valid_", "test_")))
    tr = sorted(c for k, c in HIST.items() if c not in ev)
    evaluated = hist[0, :, HIST["phase"]] != 2
    np.save(os.path.join(out_dir, "params.npy"), params)
    np.save(os.path.join(out_dir, "history_train.npy"), np.ascontiguousarray(hist[:, :, tr]))
    np.save(os.path.join(out_dir, "history_eval.npy"), np.ascontiguousarray(hist[:, evaluated][:, :, ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=210)
    ap.add_argument("--warmup", type=int, default=21)
    ap.add_argument("--models-per-gpu", type=int, default=1)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--config", choices=["real", "scaled"], default="real",
                    help="real: BASELINE config 2 (600x3000x46); scaled: config 5 (600x30000x512)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the end-to-end 9-model "
                         "ensemble wall-clock (ensemble9 in the result line)")
    ap.add_argument("--no-ensemble9", dest="ensemble9", action="store_false",
                    help="with --full: skip the end-to-end 9-model ensemble wall-clock")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step (the trained parameters and "
                         "the history rows of the timed epochs, per model of rank 0's GPU) as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    a.ensemble9 = a.ensemble9 and a.full
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(spawn_ranks(a.gpus))
    pc = SCALED if a.config == "scaled" else BENCH

    from deeplearninginassetpricing_paperreplication_amd.parallel import comm
    # RCCL ("nccl") is the production backend, one rank per GPU. DLAP_DIST_BACKEND=gloo with
    # DLAP_SHARE_GPU=1 rehearses the multi-rank path with several ranks on one GPU (RCCL refuses).
    d = comm.init(use_gpu=True)
    if d.world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the process group has {d.world} rank(s)")
    world, rank, local = d.world, d.rank, d.local_rank
    dist = d.active

    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

    if a.config == "scaled":
        a.ensemble9 = False                 # (measured separately: profiles/r1_bench_scaled_g9.json)
    t_gen = time.perf_counter()
    tr, va, te = make_panel(seed=0, device=f"cuda:{local}", cfg=pc, keep_on_device=a.config == "scaled")
    cfg = default_cli_config(pc["M"], pc["F"])
    G = a.models_per_gpu
    n1, n2, n3 = schedule_split(a.steps)
    w1, w2, w3 = schedule_split(max(a.warmup, 3))
    eng = GANEngine(AssetPricingGAN(cfg).spec, n_models=G, max_epochs=n1 + n2 + n3 + w1 + w2 + w3 + 8)
    eng.set_data(tr, va, te)
    del tr, va, te
    torch.cuda.empty_cache()
    t_gen = time.perf_counter() - t_gen
    if os.environ.get("DLAP_PIPELINE", "1") == "0":      # profiling: sequential epoch graph
        eng.eng.set_pipeline(False)
    for g in range(G):
        seed = 1000 * rank + g
        torch.manual_seed(seed)
        eng.set_model(g, AssetPricingGAN(cfg), seed)
    use_graph = not a.no_graph

    # loss mode per phase (dense or Gram, engine cost model) from the TIMED run's epoch counts, so
    # the warmup captures exactly the graphs the timed run replays
    for ph, k in ((1, n1), (2, n2), (3, n3)):
        eng.eng.plan_phase(ph, k)

    def run(k1, k2, k3):
        for ph, k in ((1, k1), (2, k2), (3, k3)):
            if k:
                eng.eng.begin_phase(ph)
                eng.run(ph, k, 1e-3, 64, 1.0, use_graph)

    run(w1, w2, w3)                       # warmup (also captures the three phase graphs)
    eng.eng.sync()
    torch.cuda.synchronize()
    comm.barrier(d)
    # the three phases are queued back to back on the engine stream (phase changes are stream-
    # ordered kernels, no host sync); per-phase times come from events on that stream
    est = torch.cuda.ExternalStream(eng.eng.stream())
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t0 = time.perf_counter()
    evs[0].record(est)
    for i, (ph, k) in enumerate(((1, n1), (2, n2), (3, n3))):
        if k:
            eng.eng.begin_phase(ph)
            eng.run(ph, k, 1e-3, 64, 1.0, use_graph)
        evs[i + 1].record(est)
    t_enq = time.perf_counter() - t0      # host time to enqueue the timed region (vs dt: host-bound?)
    launch_us = float(eng.eng.fused_info().get("host_launch_us_per_epoch", 0.0))
    eng.eng.sync()
    torch.cuda.synchronize()
    comm.barrier(d)
    dt = time.perf_counter() - t0
    phase_t = [evs[i].elapsed_time(evs[i + 1]) / 1e3 / k if k else 0.0 for i, k in enumerate((n1, n2, n3))]
    hist = eng.history_rows(0)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, eng, G, n1 + n2 + n3)
    finite = bool(np.isfinite(hist[:, 1]).all())
    # spin waits of the fused LSTM + tower forward that gave up (0 = every published period was
    # waited for; anything else means results of that launch are invalid)
    fused_timeouts = int(eng.eng.prog_timeouts())
    finite = finite and fused_timeouts == 0           # such a launch poisons its model (NaN epochs)
    K = n1 + n2 + n3
    if dist:
        dt = float(max(comm.all_gather_rows(d, np.array([[dt]]), world, [rank])[:, 0]))
    wide = bool(int(eng.desc["wide"]))
    eng_plan = {ph: eng.eng.gram_plan(ph) for ph in (1, 3)}
    del eng
    torch.cuda.empty_cache()
    ens = measure_ensemble(d, cfg, pc) if a.ensemble9 else None
    ms_per_step = dt / K * 1e3
    value = world * G * K / dt
    ref = REF_EPOCHS_PER_S_SCALED if a.config == "scaled" else REF_EPOCHS_PER_S
    # time for one model's full 256/64/1024 schedule at the measured per-phase rates
    full_s = 256 * phase_t[0] + 64 * phase_t[1] + 1024 * phase_t[2]
    if rank == 0:
        out = {
            "metric": "epochs/sec (3-phase GAN)",
            "value": round(value, 3), "unit": "model-epochs/s", "n_gpus": world, "steps": K,
            "warmup": a.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": round(value / ref, 1) if ref else None,
            "dtype": "bf16", "data": "synthetic (factor-model panel, random-init weights)",
            "config": {"model": "Chen-Pelger-Zhu GAN: LSTM[4] + SDF FFN[64,64] + 8 tanh moments",
                       "global_batch": world * G, "seq_len": pc["T_train"],
                       "panel": f"T={pc['T_train']}/{pc['T_valid']}/{pc['T_test']} "
                                f"N={pc['N']} F={pc['F']} M={pc['M']}",
                       "bench_config": a.config, "wide_layer0": wide,
                       "models_per_gpu": G, "parallelism": f"ensemble-dp{world}",
                       "backend": d.backend, "schedule_mix": [n1, n2, n3]},
            "ms_per_epoch_phase": [round(x * 1e3, 4) for x in phase_t],
            "full_schedule_s_per_model_batch": round(full_s, 3),
            "hipgraph": use_graph, "finite": finite, "fused_wait_timeouts": fused_timeouts,
            "gram_plan": [list(map(bool, eng_plan[ph])) for ph in (1, 3)],
            "panel_setup_s": round(t_gen, 2),
            "host_enqueue_ms_per_step": round(t_enq / K * 1e3, 4),
            "host_launch_us_per_epoch": round(launch_us, 1),
            "ensemble9": ens,
        }
        print(json.dumps(out), flush=True)
    comm.shutdown(d)
    if fused_timeouts:
        sys.exit("bench.py: a fused LSTM + tower forward gave up a wait -- the measurement is invalid")


if __name__ == "__main__":
    main()

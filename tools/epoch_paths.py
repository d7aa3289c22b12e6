"""The two paths of a steady split-graph epoch from a rocprofv3 --kernel-trace CSV run of bench.py:
the training chain (k_mlp_fwd_rnn -> k_period_fwd -> k_period_bwd -> k_tbwd_sdf -> k_lstm_tail) and
the evaluation graph beside it, whose k_epoch_end signals the tail's update.

Prints, over the body epochs inside an unrolled graph (epochs longer than --steady us are launch
gaps, heads or phase changes and are left out): the time from the end of k_tbwd_sdf to the end of
k_epoch_end, from there to the end of k_lstm_tail, the chain's kernel durations, k_dropmask on
the evaluation queue (n = 0 where the tail launch hashes the keep words, DLAP_TAIL_MASKS; the mask
blocks' in-kernel stamps are printed by tools/lstm_timing.py) -- then one epoch, kernel by kernel,
in us from the end of its fused forward.

Usage: python tools/epoch_paths.py <prof dir> [--epochs 45] > profiles/<name>.txt
"""
import argparse
import csv
import re
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))


def base(name):
    m = re.search(r"(k_[a-z0-9_]+(<[^>]*>)?)", name)
    return m.group(1) if m else name[:40]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--epochs", type=int, default=45, help="trailing k_lstm_tail launches to look at")
    ap.add_argument("--steady", type=float, default=170.0, help="longest epoch (us) counted as steady")
    a = ap.parse_args()
    from kernel_stats import demangle
    rows = []
    for f in Path(a.dir).glob("**/*kernel_trace.csv"):
        rows += list(csv.DictReader(open(f)))
    dm = demangle({r["Kernel_Name"] for r in rows})
    R = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), base(dm[r["Kernel_Name"]]), r["Queue_Id"])
               for r in rows)
    tails = [i for i, r in enumerate(R) if r[2].startswith("k_lstm_tail")]
    keys = ("tbwd_end_to_epoch_end_end", "epoch_end_end_to_tail_end", "chain k_period_fwd", "chain k_period_bwd",
            "k_dropmask (evaluation queue)", "epoch", "k_tbwd_sdf", "k_mlp_fwd_rnn", "k_lstm_tail")
    res = {k: [] for k in keys}
    prev_end, shown = None, None
    for i in tails[-a.epochs - 1:]:
        s, e, _, q = R[i]
        if prev_end is None or e - prev_end > a.steady * 1e3:
            prev_end = e
            continue
        win = [r for r in R if prev_end - 200000 <= r[0] <= e and r[2].startswith("k_")]
        tb = [r for r in win if r[2].startswith("k_tbwd_sdf") and r[3] == q and prev_end - 1000 <= r[0] and r[1] <= s + 1000]
        ee = [r for r in win if r[2].startswith("k_epoch_end") and r[3] != q and r[1] <= e + 20000]
        if not tb or not ee:
            prev_end = e
            continue
        tb, ee = tb[-1], max(ee, key=lambda r: r[1])
        res["tbwd_end_to_epoch_end_end"].append((ee[1] - tb[1]) / 1e3)
        res["epoch_end_end_to_tail_end"].append((e - ee[1]) / 1e3)
        res["epoch"].append((e - prev_end) / 1e3)
        res["k_tbwd_sdf"].append((tb[1] - tb[0]) / 1e3)
        res["k_lstm_tail"].append((e - s) / 1e3)
        for r in win:
            d = (r[1] - r[0]) / 1e3
            if r[3] == q and prev_end - 1000 <= r[0] <= s:
                if r[2].startswith("k_period_fwd"):
                    res["chain k_period_fwd"].append(d)
                if r[2].startswith("k_period_bwd"):
                    res["chain k_period_bwd"].append(d)
                if r[2].startswith("k_mlp_fwd_rnn"):
                    res["k_mlp_fwd_rnn"].append(d)
            if r[3] != q and r[2].startswith("k_dropmask") and tb[0] <= r[0] <= e:
                res["k_dropmask (evaluation queue)"].append(d)
        shown = (prev_end, e)
        prev_end = e
    for k in keys:
        v = res[k]
        if v:
            print(f"{k:30s} n={len(v):3d}  median {statistics.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f} us")
        else:
            print(f"{k:30s} n=  0")
    if shown:
        p, e = shown
        win = [r for r in R if p - 60000 <= r[0] <= e and r[2].startswith("k_")]
        fw = [r for r in win if r[2].startswith("k_mlp_fwd_rnn")][-1]
        print("# the last steady epoch: queue, start, end (us from the end of k_mlp_fwd_rnn), duration, kernel")
        for r in win:
            print(f"q{r[3]} {(r[0] - fw[1]) / 1e3:8.1f} {(r[1] - fw[1]) / 1e3:8.1f} {(r[1] - r[0]) / 1e3:7.1f}  {r[2]}")


if __name__ == "__main__":
    main()

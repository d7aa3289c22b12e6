"""Inputs and storage helpers shared by the tests that compare against recorded outputs of the
reference implementation (``tests/golden/``) and by the recorder ``tools/record_golden.py``.

The recorder runs the reference on exactly the inputs built here and stores what it returned;
the tests run this package on the same inputs and compare against the stored arrays, so the suite
needs no checkout of the reference. Large tensors (the shipped synthetic panel through the
reference loader) are stored as SHA-256 digests of dtype, shape and bytes: the tests they serve
assert bit equality."""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the panel the reference ships as data/synthetic_data (generate_synthetic_data.py defaults)
SHIPPED = dict(n_train=120, n_valid=30, n_test=60, n_stocks=500, n_features=46, n_macro=8, seed=42)
SHIPPED_FILES = [("char", f"Char_{s}.npz") for s in ("train", "valid", "test")] + \
                [("macro", f"macro_{s}.npz") for s in ("train", "valid", "test")]

MODEL_CONFIGS = [
    dict(),
    dict(hidden_dim=[32], rnn_dim=[2, 3], num_moments=4),
    dict(hidden_dim=[64, 48, 32], hidden_dim_moment=[16], num_moments=12),
    dict(use_lstm=False),
]
PHASES = ["unconditional", "moment", "conditional"]
GRAD_CASES = [(0.0, True), (0.5, True), (0.0, False)]
FORWARD_KEYS = ("weights", "loss", "loss_unconditional", "loss_conditional", "sharpe", "portfolio_returns",
                "moments")
TRAIN_KW = dict(num_epochs_unc=4, num_epochs_moment=2, num_epochs=5, lr=1e-3, print_freq=100, ignore_epoch=1)
CLI_COMMON = ["--small_sample", "--n_periods", "12", "--n_stocks", "40", "--epochs_unc", "3",
              "--epochs_moment", "2", "--epochs", "3", "--ignore_epoch", "0", "--print_freq", "1"]
CKPT_STATES = ("best_model_loss.pt", "best_model_sharpe.pt", "final_model.pt")


def model_batch(T=24, N=60, F=10, M=5, seed=0):
    from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
    ret, feats, mask, mac = generate_panel_fast(T, N, F, M, seed=seed)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    return mac, feats, ret, mask


def model_config(cfg_kw, residual=0.0, weighted=True):
    from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
    cfg = default_cli_config(5, 10, dropout=0.0, **cfg_kw)
    cfg["residual_loss_factor"] = residual
    cfg["weighted_loss"] = weighted
    return cfg


def residual_mask(mask):
    mask[3] = False                      # an empty period
    mask[4, 1:] = False                  # a period with one stock (skipped by the reference)
    return mask


def shipped_paths(d, s):
    return os.path.join(d, "char", f"Char_{s}.npz"), os.path.join(d, "macro", f"macro_{s}.npz")


def nan_panel_arrays(char_path):
    """The train panel with one NaN return (tests/test_data.py, memory-mapped loading)."""
    with np.load(char_path) as z:
        arrs = {k: z[k] for k in z.files}
    arrs["data"][3, 5, 0] = np.nan
    return arrs


def small_splits(data_dir, n_periods=12, n_stocks=40):
    from deeplearninginassetpricing_paperreplication_amd.data.dataset import create_small_sample, load_splits
    return [create_small_sample(d, n_periods, n_stocks) for d in load_splits(data_dir)]


# ---- storage ----------------------------------------------------------------------------
def as_numpy(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def digest(x) -> str:
    a = np.ascontiguousarray(as_numpy(x))
    h = hashlib.sha256()
    h.update(str(a.dtype).encode())
    h.update(str(tuple(a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def digests(d) -> dict:
    return {k: digest(v) for k, v in d.items()}


def path(name: str) -> str:
    return os.path.join(GOLDEN, name)


def load_json(name: str):
    with open(path(name)) as fh:
        return json.load(fh)


def load_npz(name: str) -> dict:
    with np.load(path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ulp_atol(ref, n: int = 4) -> float:
    """Absolute tolerance of ``n`` fp32 roundings at the scale of ``ref``. A recorded array was
    computed on another CPU, whose BLAS kernels sum in another order; elements much smaller than
    the tensor's largest (cancellation) then differ by roundings of the large terms, which a
    relative tolerance on the small result does not cover."""
    return n * float(np.finfo(np.float32).eps) * float(np.abs(as_numpy(ref)).max())


def tensor(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a))

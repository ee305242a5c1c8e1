"""Generate the MS-SSIM fixture by running the REFERENCE's vendored implementation
(DVC/subnet/ms_ssim_torch.py) on the seeded inputs of tests/_msssim_cases.py, on the CPU.

Run from the repo root:  python tests/golden/gen_msssim_golden.py /path/to/reference

Per case it records, per scale and image, the reference's float64 (cs, ssim) (its `_ssim` on the
planes its own pooling produces), its float64 `ms_ssim` / `ssim`, and for each of those the
reference's own |float32 - float64|: the envelope the GPU tests scale their tolerance from. It also
records the reference's float32 window taps. No pictures: the inputs are regenerated from the seed.
Asserted before writing: no value is NaN, and every cs and ssim lies in (0.05, 0.9999), so that the
clamp of negative terms (metrics.ms_ssim) cannot differ from the reference and no case is trivially 1.
Output: tests/golden/msssim_ref.json (plain data; only this file is committed).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(REPO, "tests", "golden", "msssim_ref.json")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))

import _msssim_cases as MC  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "DVC", "subnet", "ms_ssim_torch.py")
    spec = importlib.util.spec_from_file_location("ref_ms_ssim_torch", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(m, x, y, data_range, levels, dtype):
    """The reference's figures at one dtype: (scales [levels][B][2] = (cs, ssim), quality [B])."""
    X, Y = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
    win = m._fspecial_gauss_1d(11, 1.5).repeat(X.shape[1], 1, 1, 1)
    if levels == 1:
        q = m.ssim(X, Y, data_range=data_range, size_average=False)
    else:
        q = m.ms_ssim(X, Y, data_range=data_range, size_average=False)
    scales = []
    for _ in range(levels):  # the loop of the reference's ms_ssim, for its per-scale terms
        s, cs = m._ssim(X, Y, win=win, data_range=data_range, size_average=False, full=True)
        scales.append(torch.stack([cs, s], dim=-1))
        pad = (X.shape[2] % 2, X.shape[3] % 2)
        X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(scales).double().numpy(), q.double().numpy()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    m = load_reference(sys.argv[1])
    torch.set_num_threads(1)
    out = {"taps_hex": [float(v).hex() for v in m._fspecial_gauss_1d(11, 1.5).reshape(-1)], "cases": {}}
    lo, hi = 1.0, 0.0
    for case in MC.CASES:
        name, levels, B, C, h, w, kind = case
        x, y, dr = MC.make_case(case)
        s64, q64 = run(m, x, y, dr, levels, torch.float64)
        s32, q32 = run(m, x, y, dr, levels, torch.float32)
        assert not np.isnan(s64).any() and not np.isnan(q64).any() and not np.isnan(s32).any(), name
        used = np.concatenate([s64[:-1, :, 0].ravel(), s64[-1].ravel()]) if levels > 1 else s64.ravel()
        assert 0.05 < s64.min() and s64.max() < 0.9999, (name, s64.min(), s64.max())
        lo, hi = min(lo, used.min()), max(hi, used.max())
        out["cases"][name] = {"levels": levels, "shape": [B, C, h, w], "kind": kind, "data_range": dr,
                              "scales": s64.tolist(), "quality": q64.tolist(),
                              "env_scales": np.abs(s32 - s64).tolist(), "env_quality": np.abs(q32 - q64).tolist()}
        print(f"{name}: min {s64.min():.4f} max {s64.max():.6f} env<= {np.abs(s32 - s64).max():.2e} "
              f"q {q64.tolist()} env_q {np.abs(q32 - q64).max():.2e}")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", OUT, "terms in", lo, hi)


if __name__ == "__main__":
    main()

"""Build libfvc.so in-tree with hipcc for gfx950 (no JIT cache: the .so travels with the repo).

Each source compiles to its own object (in parallel, only when stale), then one link step.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = ["fvc_conv.hip", "fvc_conv_x3.hip", "fvc_deconv_x3.hip", "fvc_conv_wino.hip", "fvc_conv_wr7.hip", "fvc_conv_stem.hip", "fvc_elem.hip", "fvc_gdn.hip", "fvc_tap_gather.hip", "fvc_coder.hip",
        "fvc_iframe.hip", "fvc_torchac.hip", "fvc_pixfmt.hip", "fvc_digest.hip", "fvc_msssim.hip"]
# per-source flags: the Winograd transforms stay scalar f32 (packed f32 VALU issues slower beside MFMAs)
SRC_FLAGS = {"fvc_conv_wino.hip": ["-fno-slp-vectorize"], "fvc_conv_wr7.hip": ["-fno-slp-vectorize"]}
OUT = os.path.join(HERE, "libfvc.so")
OBJDIR = os.path.join(HERE, "build")
HEADERS = [os.path.join(HERE, "csrc", "fvc_common.h"), os.path.join(HERE, "csrc", "fvc_dist.h"),
           os.path.join(HERE, "csrc", "fvc_dx.h"), os.path.join(HERE, "csrc", "fvc_split.h"),
           os.path.join(HERE, "csrc", "fvc_taps.h"), os.path.join(os.path.dirname(HERE), "include", "fvc.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _obj(src):
    return os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, verbose):
    path = os.path.join(HERE, "csrc", src)
    obj = _obj(src)
    cmd = [_hipcc()] + FLAGS + SRC_FLAGS.get(src, []) + ["-c", path, "-o", obj + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(obj + ".tmp", obj)


def build(force=False, verbose=True):
    """Build libfvc.so and return its path."""
    os.makedirs(OBJDIR, exist_ok=True)
    todo = [s for s in SRCS if force or _stale(_obj(s), [os.path.join(HERE, "csrc", s)] + HEADERS)]
    if todo:
        with ThreadPoolExecutor(max_workers=min(len(todo), 4)) as ex:
            list(ex.map(lambda s: _compile(s, verbose), todo))
    objs = [_obj(s) for s in SRCS]
    if force or todo or _stale(OUT, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    build(force=a.force)

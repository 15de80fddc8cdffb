"""In-tree build of the gfx950 HIP kernels (plain hipcc, no hipify, no JIT
cache): produces ps_pytorch_amd/ops/libps_hip.so which travels with the repo
snapshot to GPU boxes. hipcc cross-compiles without a GPU present."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

OPS_DIR = Path(__file__).resolve().parent
KERNEL_DIR = OPS_DIR / "kernels"
SO_PATH = OPS_DIR / "libps_hip.so"
ARCH = os.environ.get("PS_ROCM_ARCH", "gfx950")

SOURCES = sorted(KERNEL_DIR.glob("*.hip"))

# f32 VALU kernels built without the packed-f32 instructions (v_pk_fma_f32
# and kin): conv_dw.hip's contract is one scalar fma chain per output, and
# conv_group_f32.hip's epilogue is scalar f32 adds
NO_PK_F32 = {"conv_dw.hip", "conv_group_f32.hip"}
NO_PK_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
OBJ_DIR = OPS_DIR / "build"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    return "hipcc"


def needs_build() -> bool:
    if not SO_PATH.exists():
        return True
    so_mtime = SO_PATH.stat().st_mtime
    deps = list(SOURCES) + list(KERNEL_DIR.glob("*.h")) + [Path(__file__)]
    return any(p.stat().st_mtime > so_mtime for p in deps)


def build(verbose: bool = True, force: bool = False) -> Path:
    if not force and not needs_build():
        return SO_PATH
    base = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC"]
    # sources of NO_PK_F32 are compiled on their own, to objects under
    # build/ (git-ignored), and linked with the rest
    objs = []
    for src in SOURCES:
        if src.name in NO_PK_F32:
            OBJ_DIR.mkdir(exist_ok=True)
            objs.append(OBJ_DIR / (src.stem + ".o"))
            _run(base + NO_PK_FLAGS + ["-c", str(src), "-o", str(objs[-1])],
                 verbose)
    # objects first: hipcc reads every input after a .hip file as HIP source
    _run(base + ["-shared", "-o", str(SO_PATH)] + [str(o) for o in objs]
         + [str(s) for s in SOURCES if s.name not in NO_PK_F32], verbose)
    return SO_PATH


def _run(cmd, verbose: bool) -> None:
    if verbose:
        print("[ps_pytorch_amd.ops.build]", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


if __name__ == "__main__":
    build(force="--force" in sys.argv)

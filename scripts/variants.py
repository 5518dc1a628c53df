#!/usr/bin/env python3
"""A/B compile-time kernel variants: `build` (here, hipcc cross-compiles) then `run` (GPU box) times cfg2 with each library.

    python scripts/variants.py build [name ...] # fastx_toolkit_amd/libfxg_v_<name>.so, git-ignored
    python scripts/variants.py run              # one JSON line per variant (scripts/ablate.py in a subprocess each)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastx_toolkit_amd import build as _b  # noqa: E402

VARIANTS = {            # edit freely: every entry becomes fastx_toolkit_amd/libfxg_v_<name>.so
    "abl": ["-DFXG_ABLATION"],
    "abl_ldnt": ["-DFXG_ABLATION", "-DFXG_ROWS_LD_AUX=2"],
    "full_bases": ["-DFXG_ROWS_SPARSE_BASES=0"],       # the rows kernels' stage B fetches every base row whole (before the sparse fetch)
    "sparse_multi": ["-DFXG_ROWS_SPARSE_BASES=2"],     # the sparse base fetch in fxg_kernel_rows_multi too
}


def lib(name):
    return os.path.join(_b.PKG, "libfxg_v_%s.so" % name)


if sys.argv[1] == "build":             # python scripts/variants.py build [name ...]: the engine's own split build and ISA check, one variant after the other
    for n in (sys.argv[2:] or VARIANTS):
        _b.compile_engine(lib(n), VARIANTS[n])
        print(n, "built", flush=True)
else:
    cfgs = os.environ.get("ABLATE") or json.dumps([["full", {}], ["decision-only", {}, False]])
    for n in (os.environ.get("VARIANTS", "").split() or VARIANTS):
        if not os.path.exists(lib(n)):
            continue
        env = dict(os.environ, FXG_LIB=lib(n), ABLATE=cfgs)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ablate.py")], env=env, capture_output=True, text=True, timeout=300)
        for line in out.stdout.splitlines():
            print(n, line, flush=True)
        if out.returncode:
            print(n, "FAILED", out.stderr[-400:], flush=True)

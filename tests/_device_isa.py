"""The emitted gfx950 device assembly of abn_api.hip (hipcc -S --cuda-device-only: cross-compiles without a GPU, ~45 s).

Shared by the ISA checks and the kernel-matrix census.  The text is cached in the temporary directory under a hash of
the sources, so one compile serves every test module of a run (and later runs on unchanged sources)."""
import hashlib
import os
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "alphabeta_rs_amd" / "csrc"


def device_isa(src=CSRC / "abn_api.hip"):
    """the assembly of `src` (compiled in its own directory); skips the calling test when hipcc is absent"""
    from alphabeta_rs_amd import build as B

    src = Path(src)
    try:
        B.hipcc_path()
    except RuntimeError as e:     # a CPU-only box without ROCm: nothing to check here (the GPU tier builds with hipcc)
        pytest.skip(str(e))
    h = hashlib.sha1()
    for f in sorted(src.parent.glob("*")):
        if f.is_file():
            h.update(f.read_bytes())
    out = Path(tempfile.gettempdir()) / f"{src.stem}_{h.hexdigest()[:16]}.s"
    if not out.exists():
        flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC", "-ldl")]
        tmp = out.with_suffix(f".{os.getpid()}.tmp")   # concurrent runs never read a half-written file
        subprocess.run([B.hipcc_path(), "-S", "--cuda-device-only", *flags, "-Wno-unused-command-line-argument", "-o",
                        str(tmp), str(src)], check=True, cwd=str(src.parent))
        tmp.replace(out)
    return out.read_text()

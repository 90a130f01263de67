"""One SHA-256 per .hip source of the Makefile's SRCS over its normalised gfx950 device assembly: the gate for an edit
that must not change what the kernels are (compare the digests of two trees).  Each source is compiled with the
Makefile's HIPFLAGS plus `-x hip -S --cuda-device-only`; the normalisation drops comments (`;` to end of line) and
blank lines and replaces the mangled names (template arguments are part of them) and the `__hip_cuid_<hash>` symbol,
which hashes the source text.  It only hashes: no instruction is inspected.
usage: python tools/device_code_digest.py <tree root> [directory to keep the normalised assembly in]"""
import hashlib
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from store_hazard_check import compile_isa  # noqa: E402


def make_vars(root):
    """The Makefile's simple `NAME := value` / `NAME ?= value` assignments, continuation lines joined, $(X) expanded."""
    text = open(os.path.join(root, "Makefile")).read().replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M):
        out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda v: out.get(v.group(1), ""), m.group(2)).strip()
    return out


def normalise(asm):
    lines = (line.split(";")[0].rstrip() for line in asm.splitlines())
    text = "\n".join(line for line in lines if line.strip()) + "\n"
    text = re.sub(r"_Z[0-9A-Za-z_$.]+", "_Z", text)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)


def digest(root, keep=None):
    """[(source name, sha256 of its normalised device assembly)] in SRCS order."""
    v = make_vars(root)
    srcs = [s for s in v["SRCS"].split() if s.endswith(".hip")]
    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1, 16)) as pool:
        texts = list(pool.map(lambda s: normalise(compile_isa(os.path.join(root, s), v["HIPFLAGS"].split())), srcs))
    if keep:
        os.makedirs(keep, exist_ok=True)
        for s, t in zip(srcs, texts):
            open(os.path.join(keep, os.path.basename(s) + ".s"), "w").write(t)
    return [(os.path.basename(s), hashlib.sha256(t.encode()).hexdigest()) for s, t in zip(srcs, texts)]


if __name__ == "__main__":
    for name, h in digest(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None):
        print(f"{h}  {name}")

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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_build import compile_all, hipflags, product_sources  # noqa: E402


def normalise(asm):
    lines = (line.split(";")[0].rstrip() for line in asm.splitlines())
    text = "\n".join(line for line in lines if line.strip()) + "\n"
    text = re.sub(r"_Z[0-9A-Za-z_$.]+", "_Z", text)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)


def digest(root, keep=None):
    """[(source name, sha256 of its normalised device assembly)] in SRCS order."""
    srcs = product_sources(root)
    texts = [normalise(b.asm) for b in compile_all(srcs, hipflags(root))]
    if keep:
        os.makedirs(keep, exist_ok=True)
        for s, t in zip(srcs, texts):
            open(os.path.join(keep, os.path.basename(s) + ".s"), "w").write(t)
    return [(os.path.basename(s), hashlib.sha256(t.encode()).hexdigest()) for s, t in zip(srcs, texts)]


if __name__ == "__main__":
    for name, h in digest(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None):
        print(f"{h}  {name}")

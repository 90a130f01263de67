"""How the product's device code is compiled, in one place: the Makefile's SRCS and HIPFLAGS, and one hipcc run per
source that returns its gfx950 assembly, its per-kernel resource usage and its warnings.  tests/test_build_hygiene.py,
tools/resource_usage.py, tools/store_hazard_check.py and tools/device_code_digest.py all compile through here, so
what they inspect is what the Makefile builds."""
import collections
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# With -S the hipcc wrapper still passes --hip-link, and the clang driver says so: the one line of a compile's
# stderr that is not about the source.
DRIVER_LINE = "clang++: warning: argument unused during compilation: '--hip-link' [-Wunused-command-line-argument]"

Build = collections.namedtuple("Build", "asm kernels warnings")
builds = {}  # (path, flags) -> Build: its length is the number of hipcc runs of this process


def make_vars(root=ROOT):
    """The Makefile's simple `NAME := value` / `NAME ?= value` assignments, continuation lines joined, $(X) expanded."""
    text = open(os.path.join(root, "Makefile")).read().replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M):
        out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda v: out.get(v.group(1), ""), m.group(2)).strip()
    return out


def product_sources(root=ROOT):
    """The .hip entries of SRCS, in order, as paths."""
    return [os.path.join(root, s) for s in make_vars(root)["SRCS"].split() if s.endswith(".hip")]


def hipflags(root=ROOT):
    """HIPFLAGS without -fPIC, which means nothing to a device-only compile."""
    return [f for f in make_vars(root)["HIPFLAGS"].split() if f != "-fPIC"]


def compile_device(path, flags=None):
    """Build(asm, kernels, warnings) of one source's device code, compiled once per (path, flags) and process; flags
    default to this tree's hipflags().  kernels: one dict per kernel instance, `name` (mangled) and the fields of
    -Rpass-analysis=kernel-resource-usage as strings (`VGPRs`, `AGPRs`, `ScratchSize [bytes/lane]`, `LDS Size
    [bytes/block]`, ...).  warnings: every line of the compiler's stderr that holds `warning:`, but DRIVER_LINE."""
    key = (os.path.abspath(path), tuple(hipflags() if flags is None else flags))
    if key not in builds:
        r = subprocess.run([HIPCC, *key[1], "-x", "hip", "--cuda-device-only", "-S", key[0], "-o", "-",
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        kernels, cur = [], None
        for line in r.stderr.splitlines():
            m = re.search(r"remark: (.*?) \[-Rpass", line)
            if not m:
                continue
            t = m.group(1).strip()
            if t.startswith("Function Name:"):
                cur = {"name": t.split(":", 1)[1].strip()}
                kernels.append(cur)
            elif cur is not None and ":" in t:
                k, v = t.split(":", 1)
                cur[k.strip()] = v.strip()
        warnings = [ln for ln in r.stderr.splitlines() if "warning:" in ln and ln != DRIVER_LINE]
        builds[key] = Build(r.stdout, kernels, warnings)
    return builds[key]


def compile_all(paths, flags=None):
    """[Build] of `paths`, compiled up to eight at a time."""
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(paths)))) as pool:
        return list(pool.map(lambda p: compile_device(p, flags), paths))


def demangle(name):
    return subprocess.run(["c++filt"], input=name, capture_output=True, text=True).stdout.strip()

"""Compares the device code of two builds of the library kernel by kernel, as text.

    python tools/isa_diff.py A B [--legacy] [--keep DIR]

A and B are device assembly files (``.s``), or source trees: a tree's ``gp_dla_detection_amd/csrc/gpdla.hip`` is compiled
device-only to assembly with the product flags of ``_lib.HIPCC_FLAGS`` (the link-stage flags left out), plus
``-DGPDLA_WITH_LEGACY`` under ``--legacy``; the two trees are compiled side by side, about a minute each.  ``--keep DIR``
writes the assembly files there (``a.s``, ``b.s``) instead of a temporary directory, so that a parent commit is compiled once.

For every kernel symbol the instruction text is compared with comments, directives and the compilation-unit id stripped
and the function number taken out of the local labels.  The tool prints the kernels that differ, with their instruction
counts and whether the sequence of opcodes is the same (only registers, offsets or immediates moved), and exits with status 1
if any kernel differs.  It compares text: it knows no instruction set.

A refactor of device code that leaves every kernel's text unchanged computes the same bits at the same speed (DESIGN.md
4.26): this is the check that decides, step by step, what such a refactor may share.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_ONLY = ("-shared", "-fPIC", "-no-hip-rt")

_TYPE = re.compile(r"^\s*\.type\s+([\w.$]+),@function")
_LABEL = re.compile(r"^([\w.$]+):")
_LOCAL = re.compile(r"\.L(BB|JTI|tmp|func_begin)\d+_")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def parse_kernels(text):
    """{symbol: [line, ...]} for every function symbol of a device assembly text: its labels and instructions, in order,
    without comments and directives."""
    kernels, name, body = {}, None, None
    for line in text.splitlines():
        line = line.split(";", 1)[0].rstrip()
        m = _TYPE.match(line)
        if m:
            name, body = m.group(1), None
            continue
        stripped = line.strip()
        if not stripped:
            continue
        m = _LABEL.match(stripped)
        if m and m.group(1) == name and body is None:
            body = kernels[name] = []
            continue
        if body is None:
            continue
        if stripped.startswith(".Lfunc_end"):
            name, body = None, None
            continue
        if m:  # a local label
            body.append(_LOCAL.sub(r".L\1_", stripped))
        elif not stripped.startswith("."):
            body.append(_CUID.sub("__hip_cuid", _LOCAL.sub(r".L\1_", " ".join(stripped.split()))))
    return kernels


def instructions(body):
    return [ln for ln in body if not ln.endswith(":")]


def opcodes(body):
    return [ln.split(None, 1)[0] for ln in instructions(body)]


def diff_kernels(a, b):
    """[(symbol, count in a or None, count in b or None, same opcode sequence)] of the kernels that differ, by name."""
    out = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            out.append((name, len(instructions(a[name])) if name in a else None,
                        len(instructions(b[name])) if name in b else None, False))
        elif a[name] != b[name]:
            out.append((name, len(instructions(a[name])), len(instructions(b[name])), opcodes(a[name]) == opcodes(b[name])))
    return out


def report(a, b, demangle=lambda s: s):
    """The report as a list of lines, and the number of differing kernels."""
    diffs = diff_kernels(a, b)
    lines = []
    for name, na, nb, same_ops in diffs:
        what = "missing in A" if na is None else "missing in B" if nb is None else \
            "same opcode sequence" if same_ops else "other opcode sequence"
        lines.append(f"DIFFERS  {demangle(name)}: {na if na is not None else '-'} -> {nb if nb is not None else '-'} instructions, {what}")
    lines.append(f"{len(set(a) | set(b))} kernels, {len(diffs)} differ")
    return lines, len(diffs)


def device_flags(legacy):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpdla_lib_flags", os.path.join(ROOT, "gp_dla_detection_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flags = [f for f in mod.HIPCC_FLAGS if f not in LINK_ONLY] + ["--cuda-device-only", "-S"]
    return flags + (["-DGPDLA_WITH_LEGACY"] if legacy else [])


def assembly_of(path, legacy, out):
    """The assembly text of a ``.s`` file, or of a source tree compiled to `out`."""
    if os.path.isdir(path):
        src = os.path.join(path, "gp_dla_detection_amd", "csrc", "gpdla.hip")
        res = subprocess.run(["hipcc", *device_flags(legacy), src, "-o", out], capture_output=True, text=True)
        if res.returncode:
            sys.exit(f"{src} does not compile:\n{res.stderr}")
        path = out
    with open(path) as f:
        return f.read()


def demangler():
    def demangle(sym):
        try:
            res = subprocess.run(["c++filt", sym], capture_output=True, text=True)
            return res.stdout.strip() or sym
        except OSError:
            return sym
    return demangle


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--legacy", action="store_true", help="compile trees with -DGPDLA_WITH_LEGACY")
    ap.add_argument("--keep", help="directory for the assembly files of compiled trees")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = args.keep or tmp
        os.makedirs(out, exist_ok=True)
        with ThreadPoolExecutor(2) as pool:
            fa = pool.submit(assembly_of, args.a, args.legacy, os.path.join(out, "a.s"))
            fb = pool.submit(assembly_of, args.b, args.legacy, os.path.join(out, "b.s"))
            a, b = parse_kernels(fa.result()), parse_kernels(fb.result())
    lines, ndiff = report(a, b, demangler())
    print("\n".join(lines))
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())

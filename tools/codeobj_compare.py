"""Compare the device code of two builds of libpmenv.so, without a GPU: a host-side change
(a refactor of the dispatch, say) must leave both equal.

    python tools/codeobj_compare.py OTHER_LIB [--lib THIS_LIB] [--arch gfx950] [--out REPORT.txt]

Compared: the set of kernel instantiations (nm -C, the __device_stub__ names with their
template arguments) and, per kernel of the arch's code object (unbundled from .hip_fatbin),
the VGPR, SGPR, LDS and scratch figures of the code object's metadata notes and the code
size (the function symbol's size). Exit status 1 on any difference."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".kernarg_segment_size", ".max_flat_workgroup_size", ".uses_dynamic_stack")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def stubs(lib):
    return {m.replace(" ", "") for m in re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", run("nm", "-C", lib))}


def kernels(lib, arch, tmp):
    """{mangled kernel name: {metadata field: value, "code_bytes": size}} of lib's code object for arch."""
    fat = os.path.join(tmp, "fat.bin")
    co = os.path.join(tmp, "code.co")
    run("objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
    targets = run(os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={fat}").split()
    target = next(t for t in targets if t.endswith(arch) or f"{arch}:" in t)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
        f"--targets={target}", f"--output={co}")
    out, recs, cur = {}, [], None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"(  - |    )(\.[a-z_]+):\s*(.*)$", line)          # a kernel's own keys: args sit deeper
        if line.startswith("  - "):
            cur = {}
            recs.append(cur)
        elif not line.startswith("    "):
            cur = None
        if m and cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'")
    for r in recs:
        if ".name" in r and ".vgpr_count" in r:
            out[r[".name"]] = {f: r.get(f) for f in FIELDS}
    sizes = {}
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            sizes[f[7]] = int(f[2], 0)
    for name, d in out.items():
        d["code_bytes"] = sizes.get(name)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--lib", default=os.path.join(ROOT, "pm-rl_amd", "pmenv", "libpmenv.so"))
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--label", default="other", help="what OTHER_LIB is (recorded), e.g. the commit it was built from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, bad = [], 0
    sa, sb = stubs(a.lib), stubs(a.other)
    lines.append(f"kernel instantiations (nm -C, __device_stub__): this build {len(sa)}, {a.label} {len(sb)}")
    for k in sorted(sa ^ sb):
        bad += 1
        lines.append(f"  only in {'this build' if k in sa else a.label}: {k}")
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ka, kb = kernels(a.lib, a.arch, ta), kernels(a.other, a.arch, tb)
    lines.append(f"{a.arch} code object kernels (metadata notes): this build {len(ka)}, {a.label} {len(kb)}")
    for k in sorted(set(ka) ^ set(kb)):
        bad += 1
        lines.append(f"  only in {'this build' if k in ka else a.label}: {k}")
    for k in sorted(set(ka) & set(kb)):
        if ka[k] != kb[k]:
            bad += 1
            diff = {f: (ka[k].get(f), kb[k].get(f)) for f in set(ka[k]) | set(kb[k]) if ka[k].get(f) != kb[k].get(f)}
            lines.append(f"  differs: {k}: {diff}")
    lines.append(f"fields compared per kernel: {', '.join(FIELDS)}, code_bytes")
    tot = lambda ks, f: sum(int(d[f]) for d in ks.values() if d.get(f) is not None)   # noqa: E731
    lines.append(f"totals, this build: code {tot(ka, 'code_bytes')} B, max vgpr "
                 f"{max(int(d['.vgpr_count']) for d in ka.values())}, max LDS "
                 f"{max(int(d['.group_segment_fixed_size']) for d in ka.values())} B, scratch "
                 f"{tot(ka, '.private_segment_fixed_size')} B")
    lines.append(f"differences: {bad}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

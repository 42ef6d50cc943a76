#!/bin/bash
# Does an edit of a kernel source change the gfx950 code hipcc makes of it?  Compiles the file as it stands at a git
# commit and as it stands in the working tree (device only, build.py's flags; the assembly carries no file names or line
# numbers), splits both by kernel -- instruction stream from the kernel's label to .Lfunc_end, and the .amdhsa_ descriptor
# block -- renumbers the local labels (.LBB<n>_<m>) and compares kernel by kernel.  Prints one line per kernel
# (instructions before / after), the first differing lines of a changed one, and exits 1 when any kernel differs.
# usage: scripts/kernel_isa_diff.sh <commit | old.s> [source = gpu-physics-engine_amd/csrc/k_native.hip] [extra flags]
# (an assembly file kept from an earlier run may stand in for the commit: KEEP=dir keeps old.s and new.s there)
set -e
old=${1:?usage: kernel_isa_diff.sh <commit | old.s> [source] [extra hipcc flags]}; shift
src=gpu-physics-engine_amd/csrc/k_native.hip
case "$1" in *.hip) src=$1; shift ;; esac
cd "$(git rev-parse --show-toplevel)"
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
out=${KEEP:-$tmp}; mkdir -p "$out"
flags=$(cd gpu-physics-engine_amd && python3 -B -c 'import build; print(*build.CXXFLAGS)')   # the library's own
asm() {   # asm <tree> <output>
    /opt/rocm/bin/hipcc $flags -Wno-unused-command-line-argument --offload-device-only -S "$1/$src" -o "$2" "${@:3}"
}
if [ -f "$old" ]; then cp "$old" "$tmp/old.s"; else
    mkdir "$tmp/tree"
    git archive "$old" gpu-physics-engine_amd/csrc include | tar -x -C "$tmp/tree"
    asm "$tmp/tree" "$tmp/old.s" "$@" &
    old_pid=$!
fi
asm . "$tmp/new.s" "$@"
[ -z "$old_pid" ] || wait "$old_pid"
[ "$out" = "$tmp" ] || cp "$tmp/old.s" "$tmp/new.s" "$out/"
python3 - "$tmp/old.s" "$tmp/new.s" <<'EOF'
import difflib, re, subprocess, sys

def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.startswith("\t.amdhsa_kernel ") or l.startswith(".amdhsa_kernel ")]
    res = {}
    for name in names:
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(lines)) if l_is_end(lines[i]))
        # (comments go: they number basic blocks and loops)
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[a:d0] + lines[d1 + 1:b]]
        body = [l for l in body if l]
        res[name] = (body, lines[d0:d1 + 1])
    return res

def l_is_end(l):
    return l.strip() == ".end_amdhsa_kernel"

def instructions(body):
    return sum(1 for l in body if l.startswith("\t") and not l.lstrip().startswith((".", ";")))

old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
changed = 0
for name in sorted(set(old) | set(new)):
    pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    if name not in old or name not in new:
        print("%-70s only in the %s build" % (pretty, "old" if name in old else "new")); changed += 1; continue
    (ob, od), (nb, nd) = old[name], new[name]
    same = ob == nb and od == nd
    print("%-70s %s  instructions %d / %d" % (pretty, "identical" if same else "DIFFERS  ", instructions(ob), instructions(nb)))
    if not same:
        changed += 1
        for l in list(difflib.unified_diff(od + ob, nd + nb, "old", "new", n=1, lineterm=""))[:40]: print("    " + l)
print("%d of %d kernels differ" % (changed, len(set(old) | set(new))))
sys.exit(1 if changed else 0)
EOF

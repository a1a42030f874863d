#!/bin/bash
# Is the device assembly of every translation unit the same as at <rev>? (compile only, no GPU needed) -- the proof a refactor of
# the kernels owes. Each tree is compiled with its own Makefile's flags; whole files are compared, less the __hip_cuid_<hash>
# symbol lines (5 per unit), which change with any edit of the source.
#   usage: tools/asm_same.sh [-k] <rev> [unit...]      (units default to every .hip of the working tree, e.g. march_baseline)
# -k: a unit whose files differ is compared KERNEL BY KERNEL, keyed by symbol: each function (its body, resource symbols and
#     kernel descriptor; the labels' function numbers, which follow the order of emission, taken out) and its metadata entry. A host
#     refactor may change the order in which the compiler emits the instantiations, or drop one that nothing launches; the unit
#     passes if it holds the same set of kernels, each identical, and the lines that belong to no kernel are the same.
set -u -o pipefail
BYKERNEL=0; [ "${1:-}" = -k ] && { BYKERNEL=1; shift; }
REV=${1:?usage: tools/asm_same.sh [-k] <rev> [unit...]}; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NEW=$ROOT/differender_amd/csrc
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
git -C "$ROOT" archive "$REV" differender_amd/csrc include | tar -x -C "$TMP" || exit 2
OLD=$TMP/differender_amd/csrc
[ $# -gt 0 ] || set -- $(cd "$NEW" && ls *.hip | sed 's/\.hip$//')

asm() {  # <tree> <unit> <out.s>
    local goal=print-common; [ "$2" = march_flat_bwdvol ] && goal=print-bwdvol
    (cd "$1" && /opt/rocm/bin/hipcc $(make -s $goal) -Wno-everything --cuda-device-only -S "$2.hip" -o - | grep -v __hip_cuid_ > "$3")
}
by_kernel() {  # <old.s> <new.s>: prints the verdict, returns 0 if same set of kernels, each identical, same remainder
    python3 - "$1" "$2" <<'EOF'
import re, sys
def split(path):
    funcs, meta, rest, cur = {}, {}, [], None
    lines = open(path).read().split("\n")
    m0, m1 = lines.index("amdhsa.kernels:"), max(i for i, l in enumerate(lines) if l.startswith("amdhsa.target:"))
    for l in lines[:m0]:
        b = re.search(r"; -- Begin function (\S+)", l)
        if b: cur = funcs.setdefault(b.group(1), [])
        if l.startswith("\t.section\t.AMDGPU.gpr_maximums"): cur = None
        if re.match(r"\t(\.section\t\.text\.|\.text$)", l): continue   # (names the NEXT function's section)
        # (BB7_3 -> BB_3 in labels and comments; the comment column moves with the number's width)
        (rest if cur is None else cur).append(re.sub(r"  +", " ", re.sub(r"(BB|func_end|func_begin)\d+", r"\1", l)))
    for e in re.split(r"\n(?=  - \.agpr_count:)", "\n".join(lines[m0 + 1:m1])):
        meta[re.search(r"\.name:\s+(\S+)", e).group(1)] = e
    return funcs, meta, [l for l in rest + lines[m1:] if not l.startswith("\t.addrsig_sym")]
(fo, mo, ro), (fn, mn, rn) = split(sys.argv[1]), split(sys.argv[2])
same = [k for k in fn if k in fo and fn[k] == fo[k] and mn.get(k) == mo.get(k)]
differ = [k for k in fn if k in fo and k not in same]
lost, added = [k for k in fo if k not in fn], [k for k in fn if k not in fo]
print("%d functions identical, %d differ, %d only at the revision, %d only here; lines outside functions %s"
      % (len(same), len(differ), len(lost), len(added), "identical" if ro == rn else "DIFFER"))
for tag, ks in (("differs", differ), ("only at the revision", lost), ("only here", added)):
    for k in ks: print("    %s: %s" % (tag, k))
sys.exit(0 if not (differ or lost or added) and ro == rn else 1)
EOF
}
make -s -C "$OLD" print-common > /dev/null   # (probes the flags once, before the parallel compiles read them)
for u in "$@"; do
    [ -f "$OLD/$u.hip" ] || { echo "$u: not in $REV"; continue; }
    while [ "$(jobs -r | wc -l)" -ge "${JOBS:-8}" ]; do wait -n; done
    { asm "$OLD" "$u" "$TMP/$u.old.s" && asm "$NEW" "$u" "$TMP/$u.new.s" || echo fail > "$TMP/$u.fail"; } &
done
wait
bad=0
for u in "$@"; do
    [ -f "$OLD/$u.hip" ] || continue
    if [ -e "$TMP/$u.fail" ]; then echo "$u: did not compile"; bad=1; continue; fi
    n=$(diff "$TMP/$u.old.s" "$TMP/$u.new.s" | grep -c '^[<>]')
    if [ "$n" -eq 0 ]; then echo "$u: identical ($(wc -l < "$TMP/$u.new.s") lines)"
    elif [ $BYKERNEL = 1 ]; then echo -n "$u: $n lines differ; by kernel: "; by_kernel "$TMP/$u.old.s" "$TMP/$u.new.s" | c++filt || bad=1
    else echo "$u: $n lines differ"; bad=1; fi
    [ -n "${KEEP:-}" ] && cp "$TMP/$u.old.s" "$TMP/$u.new.s" "$KEEP/"
done
exit $bad

#!/bin/bash
# Is the device assembly of every translation unit the same as at <rev>? (compile only, no GPU needed) -- the proof a refactor of
# the kernels owes. Each tree is compiled with its own Makefile's flags; whole files are compared, less the __hip_cuid_<hash>
# symbol lines (5 per unit), which change with any edit of the source.
#   usage: tools/asm_same.sh <rev> [unit...]      (units default to every .hip of the working tree, e.g. march_baseline)
set -u
REV=${1:?usage: tools/asm_same.sh <rev> [unit...]}; shift
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
    if [ "$n" -eq 0 ]; then echo "$u: identical ($(wc -l < "$TMP/$u.new.s") lines)"; else echo "$u: $n lines differ"; bad=1; fi
    [ -n "${KEEP:-}" ] && cp "$TMP/$u.old.s" "$TMP/$u.new.s" "$KEEP/"
done
exit $bad

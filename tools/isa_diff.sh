#!/bin/bash
# Compare the gfx950 machine code of every kernel in csrc/k_*.hip between a git revision and the working tree: the check
# that a refactor leaves the shipped code objects alone.  No GPU needed.  One line per kernel on stdout: `identical`, or the
# instruction counts before -> after and the resource lines that differ (descriptor and metadata: registers, spills,
# scratch, LDS).  Exit status 1 if any kernel differs.
# usage: tools/isa_diff.sh <rev> [extra hipcc flags...]          (HIPCC, JOBS from the environment)
set -e
rev="${1:?usage: tools/isa_diff.sh <rev> [extra hipcc flags...]}"; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
tmp="$(mktemp -d /tmp/dvs_isa_XXXXXX)"
trap 'git -C "$root" worktree remove --force "$tmp/old" 2>/dev/null || true; rm -rf "$tmp"' EXIT
git -C "$root" worktree prune
git -C "$root" worktree add -f --detach "$tmp/old" "$rev" >/dev/null
flags="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-value -Wno-unused-command-line-argument $* --cuda-device-only -S"      # csrc/Makefile CXXFLAGS
mkdir -p "$tmp/a" "$tmp/b"
(cd "$root/dags_vae_search_amd/csrc" && ls k_*.hip) | xargs -P "${JOBS:-8}" -I{} sh -c \
    "${HIPCC:-/opt/rocm/bin/hipcc} $flags '$tmp/old/dags_vae_search_amd/csrc/{}' -o '$tmp/a/{}.s' 2>/dev/null || true
     ${HIPCC:-/opt/rocm/bin/hipcc} $flags '$root/dags_vae_search_amd/csrc/{}' -o '$tmp/b/{}.s'"
# one file per kernel symbol: <sym>.isa = instruction text from the symbol's label to its end label (comments dropped),
# <sym>.res = its .amdhsa_* descriptor lines and the resource lines of its metadata entry.  Block labels lose the
# function's ordinal in the file (.LBB12_3 -> .LBB_3), so moving a kernel within its file changes nothing
split() {
    awk -v out="$2" '
        function flush(   i) { if (mname != "") for (i = 0; i < nm; ++i) print mline[i] >> (out "/" mname ".res"); nm = 0; mname = "" }
        /^\t\.type\t.*,@function/ { fn = $2; sub(/,.*/, "", fn) }
        /^[A-Za-z_][A-Za-z0-9_$.]*:/ { sym = $1; sub(/:.*/, "", sym); code = (sym == fn); next }
        /^\.Lfunc_end[0-9]+:/ { code = 0 }
        /^\t\.amdhsa_kernel / { kd = $2; next }
        /^\t\.end_amdhsa_kernel/ { kd = ""; next }
        kd != "" { print > (out "/" kd ".res"); next }
        /^\t\.section/ { code = 0 }
        code { sub(/[ \t]*;.*/, ""); gsub(/\.LBB[0-9]+_/, ".LBB_"); if ($0 != "") print > (out "/" sym ".isa") }
        /^  - \./ { flush() }
        /^    \.name:/ { mname = $2 }
        /^(  - |    )\.(agpr_count|vgpr_count|sgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):/ { sub(/^  - /, "    "); mline[nm++] = $0 }
        /^\t\.end_amdgpu_metadata/ { flush() }' "$1"
}
status=0
for s in "$tmp"/b/*.s; do
    f="$(basename "$s" .s)"
    mkdir -p "$tmp/ka/$f" "$tmp/kb/$f"
    [ -f "$tmp/a/$f.s" ] && split "$tmp/a/$f.s" "$tmp/ka/$f"
    split "$s" "$tmp/kb/$f"
    for k in $( (cd "$tmp/ka/$f" && ls; cd "$tmp/kb/$f" && ls) | sed -n 's/\.isa$//p' | sort -u); do
        touch "$tmp/ka/$f/$k.res" "$tmp/kb/$f/$k.res"
        name="$(echo "$k" | (c++filt 2>/dev/null || cat) | sed 's/(.*//; s/^void //')"
        if [ ! -f "$tmp/ka/$f/$k.isa" ]; then echo "$f  $name  only in the working tree"; status=1; continue; fi
        if [ ! -f "$tmp/kb/$f/$k.isa" ]; then echo "$f  $name  only in $rev"; status=1; continue; fi
        if cmp -s "$tmp/ka/$f/$k.isa" "$tmp/kb/$f/$k.isa" && cmp -s "$tmp/ka/$f/$k.res" "$tmp/kb/$f/$k.res"; then
            echo "$f  $name  identical"; continue
        fi
        status=1
        na=$(grep -c $'^\t[a-z]' "$tmp/ka/$f/$k.isa"); nb=$(grep -c $'^\t[a-z]' "$tmp/kb/$f/$k.isa")
        if cmp -s "$tmp/ka/$f/$k.res" "$tmp/kb/$f/$k.res"; then echo "$f  $name  stream differs: $na -> $nb instructions; resource lines unchanged"
        else echo "$f  $name  DIFFERS: $na -> $nb instructions; resource lines:"; diff "$tmp/ka/$f/$k.res" "$tmp/kb/$f/$k.res" | sed -n 's/^[<>]/     &/p'; fi
    done
done
exit $status

#!/usr/bin/env bash
# device_code_diff.sh LIB_A LIB_B -- is the gfx950 device code of two builds of the library the same?
#
# From each .so: the .hip_fatbin section, from it the hipv4-amdgcn-amd-amdhsa--gfx950 code object; then the SHA-1 of its .text and of
# its .rodata, and its symbol table as (name, size) without the __hip_cuid_<hash> symbol (a hash of the source text).  Prints
# "identical", or the sections whose hashes differ and the symbols that are in one table only or differ in size; exit status 1 then.
# For host-side refactors: equal device code means no kernel was added, lost or compiled differently.  No GPU.
set -euo pipefail
[ $# -eq 2 ] || { echo "usage: $0 LIB_A LIB_B" >&2; exit 2; }
LLVM=${ROCM_LLVM:-${ROCM_PATH:-/opt/rocm}/llvm/bin}
TARGET=hipv4-amdgcn-amd-amdhsa--gfx950
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT

extract() {  # extract LIB NAME -> $tmp/NAME.{text,rodata,syms}
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$tmp/$2.fatbin" "$1" "$tmp/$2.stripped"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets="$TARGET" --input="$tmp/$2.fatbin" --output="$tmp/$2.co"
  "$LLVM/llvm-objcopy" --dump-section .text="$tmp/$2.text" --dump-section .rodata="$tmp/$2.rodata" "$tmp/$2.co" "$tmp/$2.co.out"
  "$LLVM/llvm-readobj" --elf-output-style=GNU --symbols "$tmp/$2.co" |
    awk '$1 ~ /^[0-9]+:$/ && NF == 8 && $7 != "UND" && $8 !~ /^__hip_cuid_/ { print $8, $3 }' | sort > "$tmp/$2.syms"
}
extract "$1" a
extract "$2" b

status=0
for sec in text rodata; do
  ha=$(sha1sum < "$tmp/a.$sec" | cut -d' ' -f1)
  hb=$(sha1sum < "$tmp/b.$sec" | cut -d' ' -f1)
  echo ".$sec  $ha  $hb"
  [ "$ha" = "$hb" ] || { echo ".$sec differs"; status=1; }
done
echo "symbols  $(wc -l < "$tmp/a.syms")  $(wc -l < "$tmp/b.syms")"
if ! diff "$tmp/a.syms" "$tmp/b.syms" > "$tmp/syms.diff"; then
  echo "symbols (name size) that differ, < $1, > $2:"
  cat "$tmp/syms.diff"
  status=1
fi
[ $status -eq 0 ] && echo identical
exit $status

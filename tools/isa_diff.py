"""Compare the disassembly of every kernel symbol of an OLD libiqlhip.so with the same symbol in a NEW one.

    python tools/isa_diff.py OLD.so NEW.so [--out FILE]

Per symbol of OLD: the instruction text of its llvm-objdump -d (no raw bytes, no addresses; branch targets as
symbolic labels) must equal NEW's.  Symbols only NEW has are listed as added.  Exit status 1 when any old symbol
changed or is missing.  Runs without a GPU."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def functions(lib: str) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        fat, dev = os.path.join(tmp, "fatbin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib,
                        os.path.join(tmp, "copy.so")], check=True)
        subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}"], check=True)
        text = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                               "--symbolize-operands", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:", line)
        if m and not re.fullmatch(r"L\d+", m.group(1)):
            cur = funcs.setdefault(m.group(1), [])
        elif m and cur is not None:
            cur.append(f"<{m.group(1)}>:")
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].rstrip())
    # local labels (L<n>) are numbered across the whole object: renumber them per function in order of appearance
    # (and drop the alignment padding behind the last instruction: it depends on where the next function starts)
    for name, ins in funcs.items():
        while ins and ins[-1].strip() in ("s_nop 0", "s_code_end", "..."):
            ins.pop()
        ids = {}
        funcs[name] = [re.sub(r"\bL\d+\b", lambda m: "L%d" % ids.setdefault(m.group(0), len(ids)), x) for x in ins]
    return funcs


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--out")
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    lines, bad = [], 0
    for name in sorted(old):
        if name not in new:
            lines.append(f"MISSING {name}")
            bad += 1
        elif old[name] != new[name]:
            lines.append(f"CHANGED {name} ({len(old[name])} -> {len(new[name])} lines)")
            bad += 1
    added = sorted(set(new) - set(old))
    summary = (f"{len(old)} symbols in the old code object, {len(old) - bad} with identical disassembly, "
               f"{bad} changed or missing; {len(added)} added")
    out = [summary] + lines + [f"added {n}" for n in added]
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

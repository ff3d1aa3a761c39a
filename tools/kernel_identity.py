#!/usr/bin/env python3
"""Compare the disassembly of two builds of the env's device code, function by function.

    python tools/kernel_identity.py A/libcda_hip.so B/libcda_hip.so
    (or two outputs of `hipcc <the build's flags> --cuda-device-only -c csrc/cda_hip.hip`: the first AMDGPU code object found in each file is compared)

Every function of A (kernels and out-of-line device functions) is looked up in B under the same mangled name; its instruction text is compared
after dropping addresses and the `// <address>` comments (branch offsets are relative, so they compare as they are) and what only says WHERE a
function lies or which kernels exist beside it: the pc-relative literal behind s_getpc_b64 (the distance to a callee or a table), the ordinal of the
calling kernel that a call passes in s15 (the module's LDS kernel id: it counts every kernel of the code object), the alignment padding (s_nop, or the zero
fill objdump prints as "...") behind a function's last instruction.
Prints one line per function that differs or is missing, the functions only B has, and a summary; exit status 1 if a function of A differs.
Also compares the kernels' metadata (registers, spills, scratch, LDS, kernarg size)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import code_objects  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def bodies(co):
    asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for name, body in out.items():
        # ("...": the zero fill objdump elides between a function and the next one's alignment; a single zero word it prints as the instruction 0x00000000 decodes to -
        #  no function ends on a v_cndmask)
        while body and (body[-1].startswith("s_nop") or body[-1] in ("...", "v_cndmask_b32_e32 v0, s0, v0, vcc")):
            body.pop()
        for i, ins in enumerate(body):                       # s15 set within a few instructions of a call: the kernel's ordinal
            if re.match(r"s_mov_b32 s15, \d+$", ins) and any("s_swappc_b64" in x for x in body[i + 1:i + 160]):
                body[i] = "s_mov_b32 s15, <kernel id>"
        for i, ins in enumerate(body):
            if ins.startswith("s_getpc_b64"):
                for j in range(i + 1, min(i + 4, len(body))):
                    if re.match(r"s_add_u32 (s\d+|vcc_lo), \1, 0x[0-9a-f]+$", body[j]):
                        body[j] = re.sub(r"0x[0-9a-f]+$", "<pcrel>", body[j])
    return out


def metadata(co):
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                     for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")}
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cos = []
        for k, path in enumerate(sys.argv[1:3]):
            cos.append(os.path.join(tmp, "%d.co" % k))
            with open(cos[-1], "wb") as fh:
                fh.write(code_objects(path)[0])
        a, b = bodies(cos[0]), bodies(cos[1])
        ma, mb = metadata(cos[0]), metadata(cos[1])
    same = diff = missing = 0
    for name in sorted(a):
        if name not in b:
            missing += 1
            print("MISSING in B: %s" % name)
        elif a[name] != b[name]:
            diff += 1
            print("DIFFERS: %s (%d vs %d instructions)" % (name, len(a[name]), len(b[name])))
        else:
            same += 1
    meta_diff = [n for n in sorted(ma) if n in mb and ma[n] != mb[n]]
    for n in meta_diff:
        print("METADATA DIFFERS: %s %r vs %r" % (n, ma[n], mb[n]))
    new = sorted(n for n in b if n not in a)
    print("functions of A: %d   identical in B: %d   different: %d   missing: %d   kernels with different metadata: %d" % (len(a), same, diff, missing, len(meta_diff)))
    print("functions only in B: %d" % len(new))
    for n in new:
        print("  + %s (%d instructions)%s" % (n, len(b[n]), "  %r" % mb[n] if n in mb else ""))
    return 1 if diff or missing or meta_diff else 0


if __name__ == "__main__":
    sys.exit(main())

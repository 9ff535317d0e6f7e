#!/usr/bin/env python3
"""Wait-state audit of gfx950 machine code: a second opinion on the hazard padding of the code object that ships.

The kernels do not ship as the compiler left them: tools/isa_resched.py re-orders their vector instructions and pads
the hazards it creates with its own rules.  This audit shares no code with that pass.  Its rule table is written from
the CDNA3 / CDNA4 ISA's table of wait states that software must insert (section "Manually Inserted Wait States"):

    first instruction                                second instruction                                      wait states
    VALU writes an SGPR or VCC                       VALU reads it (explicit operand, or VCC implicitly)          2
    VALU writes an SGPR or VCC                       VMEM reads it                                                5
    VALU writes an SGPR or VCC                       v_readlane / v_writelane reads it as the lane select         4
    VALU writes EXEC (v_cmpx)                        v_readlane / v_readfirstlane / v_writelane                   4
    VALU writes VCC                                  v_div_fmas                                                   4
    VALU writes a VGPR                               v_readlane / v_readfirstlane reads it                        1
    VALU writes a VGPR                               DPP reads it                                                 2
    VALU writes EXEC                                 DPP                                                          5
    transcendental op, SDWA with dst_sel other       any VALU reads it                                            1
      than DWORD, or VOP3 with a dst op_sel, writes a VGPR
    SALU writes M0                                   LDS DMA (global/buffer ... lds), s_sendmsg, lds_direct       1

A wait state is one instruction issued; `s_nop N` is N + 1.  Each function is walked as one straight line: state is
reset only where a function starts and is kept across labels and branch targets, which is conservative for code that
falls through.  Only the most recent VALU writer of a register counts, and a later SALU or memory write does not
clear it (so a read that the hardware would take from the later writer can still be flagged: stricter, never laxer).

Input: a shared library with a .hip_fatbin section (its gfx950 code object is unbundled), an AMDGPU ELF (code object or
relocatable object), or assembly text (directives, labels and comments are skipped; ;;#ASMSTART / ;;#ASMEND are
comments like any other).  The compiler's own text must audit clean: a rule that flags it is wrong.

    python tools/isa_audit.py neuron_poker_amd/libmcq_hip.so      # exit status 1 on any violation
    python tools/isa_audit.py build/mcq_kernels.s --functions     # also list every function walked
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("MCQ_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

VALU_SGPR_VALU = 2
VALU_SGPR_VMEM = 5
VALU_SGPR_LANESEL = 4
VALU_EXEC_LANE = 4
VALU_VCC_DIV_FMAS = 4
VALU_VGPR_READLANE = 1
VALU_VGPR_DPP = 2
VALU_EXEC_DPP = 5
FORWARD_VALU = 1
SALU_M0_LDS = 1

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
VMEM = ("global_", "buffer_", "flat_", "scratch_", "tbuffer_")
# VALU instructions with a second destination (a carry-out or a 64-bit mask in an SGPR pair / VCC)
TWO_DST = ("v_add_co_u32", "v_sub_co_u32", "v_subrev_co_u32", "v_addc_co_u32", "v_subb_co_u32", "v_subbrev_co_u32",
           "v_div_scale_f32", "v_div_scale_f64", "v_mad_u64_u32", "v_mad_i64_i32")
NO_DST = ("v_nop",)

_REG = re.compile(r"(?<![\w.])(?:([vsa])\[(\d+):(\d+)\]|([vsa])(\d+)(?!\w)|(vcc_lo|vcc_hi|vcc|exec_lo|exec_hi|exec|m0)(?!\w))")
_ALIAS = {"vcc": ("vcc_lo", "vcc_hi"), "exec": ("exec_lo", "exec_hi"), "s106": ("vcc_lo",), "s107": ("vcc_hi",)}


def regs(text):
    """the registers an operand names, 32-bit pieces: v0, s4, a1, vcc_lo, vcc_hi, exec_lo, exec_hi, m0"""
    out = []
    for m in _REG.finditer(text):
        if m.group(1):
            names = ["%s%d" % (m.group(1), k) for k in range(int(m.group(2)), int(m.group(3)) + 1)]
        elif m.group(4):
            names = ["%s%s" % (m.group(4), m.group(5))]
        else:
            names = [m.group(6)]
        for n in names:
            out.extend(_ALIAS.get(n, (n,)))
    return out


def operands(args):
    """split an operand list at top-level commas; modifiers behind the last operand (`bitop3:0xfe`, `dst_sel:WORD_1`,
    `offset:16`, `op_sel:[0,1]` ...) are returned separately"""
    parts, depth, cur = [], 0, ""
    for ch in args:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    cur = cur.strip()
    mods = ""
    if cur:
        # the last operand ends at the first blank outside brackets and |..|
        depth, cut = 0, None
        for i, ch in enumerate(cur):
            if ch in "[(":
                depth += 1
            elif ch in "])":
                depth -= 1
            elif ch == " " and depth == 0:
                cut = i
                break
        if cut is not None:
            cur, mods = cur[:cut], cur[cut + 1:]
        parts.append(cur)
    if len(parts) == 1 and re.fullmatch(r"[a-z_]+:.*", parts[0]):  # only modifiers (s_waitcnt-like forms)
        return [], parts[0]
    return parts, mods


def is_sgpr(r):
    return r.startswith(("s", "vcc_", "exec_")) or r == "m0"


def is_vgpr(r):
    return r[0] == "v" and r[1:].isdigit()


class Ins:
    __slots__ = ("op", "args", "where", "text", "reads", "writes", "lanesel")

    def __init__(self, op, args, where, text):
        self.op, self.args, self.where, self.text = op, args, where, text
        ops, mods = operands(args)
        self.reads, self.writes, self.lanesel = set(), set(), set()
        base = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
        if op.startswith("v_"):
            n_dst = 0 if base in NO_DST else 2 if base in TWO_DST else 1
            for k, o in enumerate(ops):
                (self.writes if k < n_dst else self.reads).update(regs(o))
            if base.startswith("v_cmpx"):
                self.writes.update(("exec_lo", "exec_hi"))
            if base.startswith(("v_readlane", "v_writelane")) and len(ops) >= 3:
                self.lanesel.update(regs(ops[2]))
            if base.startswith("v_div_fmas"):
                self.reads.update(("vcc_lo", "vcc_hi"))
            if base.startswith("v_writelane") or "UNUSED_PRESERVE" in mods:
                self.reads |= self.writes  # a partial write reads its destination
        elif op.startswith("s_") and ops and op not in ("s_nop", "s_waitcnt") and not op.startswith(
                ("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_sendmsg", "s_set", "s_barrier",
                 "s_endpgm", "s_wait", "s_sleep", "s_trap", "s_ttrace")):
            self.writes.update(regs(ops[0]))
            for o in ops[1:]:
                self.reads.update(regs(o))
        else:
            for o in ops:
                self.reads.update(regs(o))
        self.reads.discard("")

    def ws(self):
        """wait states this instruction provides"""
        if self.op == "s_nop":
            m = re.match(r"\s*(0x[0-9a-fA-F]+|\d+)", self.args)
            return (int(m.group(1), 0) if m else 0) + 1
        return 1


def forwards(ins):
    """True if a VGPR this VALU instruction writes must not be read by the very next VALU instruction"""
    if ins.op.startswith(TRANS):
        return True
    if ins.op.endswith("_sdwa") and "dst_sel:" in ins.args and "dst_sel:DWORD" not in ins.args:
        return True
    m = re.search(r"\bop_sel:\[([01,]+)\]", ins.args)
    if m and ins.op.startswith("v_") and not ins.op.startswith("v_pk_"):
        bits = m.group(1).split(",")
        ops, _ = operands(ins.args)
        return len(bits) == len(ops) and bits[-1] == "1"  # one bit per source and a last one for the destination
    return False


def walk(func, body):
    """body: list of Ins of ONE function in program order.  Returns a list of violations."""
    bad = []
    ws = 0
    valu_w = {}   # register -> (wait-state count after the VALU instruction that wrote it last, that instruction)
    fwd_w = {}    # VGPR -> same, when that writer forwards (transcendental / partial-dst)
    salu_m0 = None

    def need(table, r, n, rule, ins):
        if r in table:
            end, w = table[r]
            have = ws - end
            if have < n and not (bad and bad[-1]["where"] == ins.where and bad[-1]["rule"] == rule):  # once per pair
                bad.append({"function": func, "where": ins.where, "first_where": w.where, "first": w.text,
                            "second": ins.text, "rule": rule, "register": r, "have": have, "need": n})

    for ins in body:
        op = ins.op
        if op.startswith("v_"):
            lane = op.startswith(("v_readlane", "v_readfirstlane"))
            rwlane = lane or op.startswith("v_writelane")
            dpp = op.endswith("_dpp") or "quad_perm:" in ins.args or "row_" in ins.args
            for r in ins.reads:
                if is_sgpr(r) and not r.startswith("exec"):
                    need(valu_w, r, VALU_SGPR_VALU, "VALU writes SGPR/VCC -> VALU reads it", ins)
                if is_vgpr(r):
                    if lane:
                        need(valu_w, r, VALU_VGPR_READLANE, "VALU writes VGPR -> v_readlane/v_readfirstlane reads it", ins)
                    if dpp:
                        need(valu_w, r, VALU_VGPR_DPP, "VALU writes VGPR -> DPP reads it", ins)
                    need(fwd_w, r, FORWARD_VALU, "transcendental/partial-dst VALU writes VGPR -> VALU reads it", ins)
            for r in ins.lanesel:
                if is_sgpr(r):
                    need(valu_w, r, VALU_SGPR_LANESEL, "VALU writes SGPR -> lane select reads it", ins)
            if rwlane:
                for r in ("exec_lo", "exec_hi"):
                    need(valu_w, r, VALU_EXEC_LANE, "VALU writes EXEC -> v_readlane/v_readfirstlane/v_writelane", ins)
            if dpp:
                for r in ("exec_lo", "exec_hi"):
                    need(valu_w, r, VALU_EXEC_DPP, "VALU writes EXEC -> DPP", ins)
            if op.startswith("v_div_fmas"):
                for r in ("vcc_lo", "vcc_hi"):
                    need(valu_w, r, VALU_VCC_DIV_FMAS, "VALU writes VCC -> v_div_fmas", ins)
        elif op.startswith(VMEM):
            for r in ins.reads:
                if is_sgpr(r):
                    need(valu_w, r, VALU_SGPR_VMEM, "VALU writes SGPR -> VMEM reads it", ins)
        if (op.startswith(VMEM) and "_lds" in op) or op.startswith(("s_sendmsg", "ds_read_addtid", "ds_write_addtid")) \
                or "lds_direct" in ins.args:
            if salu_m0 is not None and ws - salu_m0[0] < SALU_M0_LDS:
                bad.append({"function": func, "where": ins.where, "first_where": salu_m0[1].where,
                            "first": salu_m0[1].text, "second": ins.text,
                            "rule": "SALU writes M0 -> LDS DMA / s_sendmsg", "register": "m0",
                            "have": ws - salu_m0[0], "need": SALU_M0_LDS})
        ws += ins.ws()
        if op.startswith("v_"):
            f = forwards(ins)
            for r in ins.writes:
                valu_w[r] = (ws, ins)
                if is_vgpr(r):
                    if f:
                        fwd_w[r] = (ws, ins)
                    else:
                        fwd_w.pop(r, None)
        elif op.startswith("s_") and "m0" in ins.writes:
            salu_m0 = (ws, ins)
    return bad


# ------------------------------------------------------------------------------------------ input
_OBJDUMP_FUNC = re.compile(r"^([0-9a-fA-F]+) <(.+)>:\s*$")
_OBJDUMP_INS = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b([^/]*?)\s*//\s*([0-9A-Fa-f]+):")
_ASM_INS = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b(.*)$")


def parse_objdump(text):
    """llvm-objdump -d output -> {function: [Ins]}"""
    funcs, cur = {}, None
    for line in text.splitlines():
        m = _OBJDUMP_FUNC.match(line)
        if m:
            cur = funcs.setdefault(m.group(2), [])
            continue
        m = _OBJDUMP_INS.match(line)
        if m and cur is not None:
            op, args, off = m.group(1), m.group(2).strip(), m.group(3)
            cur.append(Ins(op, args, "0x%X" % int(off, 16), (op + " " + args).strip()))
    return funcs


def parse_asm(lines):
    """assembly text -> {function: [Ins]}; a function runs from its label to its .Lfunc_end label (or the next function)"""
    funcs, cur = {}, None
    declared = set()
    for n, line in enumerate(lines, 1):
        s = line.rstrip("\n")
        m = re.match(r"^\s*\.type\s+([^,\s]+)\s*,\s*@function", s)
        if m:
            declared.add(m.group(1))
            continue
        m = re.match(r"^([^\s:;]+):", s)
        if m:
            if m.group(1) in declared:
                cur = funcs.setdefault(m.group(1), [])
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        m = _ASM_INS.match(s)
        if not m or s.lstrip().startswith((".", ";", "//")):
            continue
        op, args = m.group(1), re.sub(r"\s*(;|//).*$", "", m.group(2)).strip()
        cur.append(Ins(op, args, "line %d" % n, (op + " " + args).strip()))
    return funcs


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        raise SystemExit("%s failed:\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return r.stdout


def code_object(path, tmp):
    """path of an AMDGPU ELF for `path`: itself, or the gfx950 code object unbundled from its .hip_fatbin"""
    hdr = _run([LLVM + "/llvm-readelf", "-h", path])
    if "AMDGPU" in hdr:
        return path
    fb = os.path.join(tmp, "fatbin.bin")
    _run([LLVM + "/llvm-objcopy", "--dump-section=.hip_fatbin=" + fb, path, os.path.join(tmp, "stripped")])
    co = os.path.join(tmp, "kernels.co")
    _run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fb,
          "--output=" + co])
    return co


def kernel_descriptors(co):
    """names of the kernels a code object declares (its distinct `<name>.kd` symbols), without the suffix"""
    out = _run([LLVM + "/llvm-readelf", "--syms", "--wide", co])
    return {w[-1][:-3] for w in (l.split() for l in out.splitlines()) if w and w[-1].endswith(".kd")}


def load(path):
    """{function: [Ins]} and the kernel-descriptor names (None for assembly text)"""
    with open(path, "rb") as f:
        magic = f.read(4)
    if magic != b"\x7fELF":
        with open(path) as f:
            return parse_asm(f.readlines()), None
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(path, tmp)
        dis = _run([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", co])
        return parse_objdump(dis), kernel_descriptors(co)


def audit(path):
    """(functions walked {name: instruction count}, kernel descriptors or None, violations)"""
    funcs, kds = load(path)
    bad = []
    for name, body in funcs.items():
        bad.extend(walk(name, body))
    return {k: len(v) for k, v in funcs.items()}, kds, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("path", help="libmcq_hip.so, a code object / object file, or a .s file")
    ap.add_argument("--functions", action="store_true", help="list every function walked and its instruction count")
    a = ap.parse_args()
    funcs, kds, bad = audit(a.path)
    if a.functions:
        for name, n in funcs.items():
            print("%8d  %s" % (n, name))
    for v in bad:
        print("%s: %s (%s: %d wait states, %d needed)\n    %-10s %s\n    %-10s %s" % (
            v["function"], v["rule"], v["register"], v["have"], v["need"], v["first_where"], v["first"], v["where"],
            v["second"]))
    extra = "" if kds is None else ", %d kernel descriptors" % len(kds)
    print("isa_audit: %s: %d functions, %d instructions%s, %d violations" % (
        os.path.basename(a.path), len(funcs), sum(funcs.values()), extra, len(bad)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

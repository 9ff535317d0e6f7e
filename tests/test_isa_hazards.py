"""tools/isa_audit.py -- the wait-state audit of the code object that ships in libmcq_hip.so (csrc/Makefile runs it on
every build).  Its rules are checked on hand-written sequences, assembled for gfx950: each rule one wait state short
(flagged) and exactly padded (clean).  Then the compiler's own text, and the code object inside the library, must audit
clean, with every kernel walked."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_audit as A  # noqa: E402

BUILD = os.path.join(ROOT, "neuron_poker_amd", "csrc", "build")
LIB = os.path.join(ROOT, "neuron_poker_amd", "libmcq_hip.so")
built = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(BUILD, "mcq_kernels.s"))),
                           reason="the library has not been built here")

# (name, writer, reader, wait states the reader needs behind the writer)
RULES = [
    ("sgpr_valu", ["v_readlane_b32 s1, v127, 45"], "v_xor_b32_e32 v4, s1, v4", 2),
    ("vcc_valu", ["v_cmp_eq_u32_e32 vcc, 0, v6"], "v_cndmask_b32_e32 v1, v2, v3, vcc", 2),
    ("carry_valu", ["v_add_co_u32_e64 v1, s[4:5], v2, v3"], "v_cndmask_b32_e64 v5, v6, v7, s[4:5]", 2),
    ("carry_in_valu", ["v_add_co_u32_e32 v1, vcc, v2, v3"], "v_addc_co_u32_e32 v4, vcc, 0, v5, vcc", 2),
    ("sgpr_vmem", ["v_readfirstlane_b32 s4, v1"], "global_load_dword v2, v3, s[4:5]", 5),
    ("sgpr_lanesel", ["v_readfirstlane_b32 s4, v1"], "v_readlane_b32 s5, v2, s4", 4),
    ("sgpr_writelane_sel", ["v_readfirstlane_b32 s4, v1"], "v_writelane_b32 v2, 7, s4", 4),
    ("exec_lane", ["v_cmpx_eq_u32_e64 s[6:7], v1, v2"], "v_readfirstlane_b32 s4, v3", 4),
    ("vgpr_readlane", ["v_add_u32_e32 v1, v2, v3"], "v_readlane_b32 s4, v1, 3", 1),
    ("vgpr_readfirstlane", ["v_add_u32_e32 v1, v2, v3"], "v_readfirstlane_b32 s4, v1", 1),
    ("vgpr_dpp", ["v_mov_b32_e32 v1, v2"], "v_add_u32_dpp v3, v1, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", 2),
    ("trans", ["v_rcp_f32_e32 v1, v2"], "v_mul_f32_e32 v3, v1, v4", 1),
    ("sdwa_partial", ["v_add_u32_sdwa v1, v2, v3 dst_sel:WORD_1 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD"],
     "v_add_u32_e32 v4, v1, v5", 1),
    ("m0_lds_dma", ["s_mov_b32 m0, s2"], "global_load_lds_dwordx4 v[0:1], off", 1),
]
# the sequence the post-pass produced in the small-batch kernels: the read of s1 sits one wait state behind its write,
# with the comment pair of an `asm volatile("")` barrier in between
QUOTED = ["v_readlane_b32 s1, v127, 45", ";;#ASMSTART", ";;#ASMEND", "s_nop 0", "v_xor_b32_e32 v4, s1, v4",
          "v_mad_u64_u32 v[2:3], s[24:25], v5, s7, 0"]
QUOTED_FIXED = QUOTED[:3] + ["s_nop 1"] + QUOTED[4:]


def pad(n, filler=False):
    """n wait states: one s_nop (s_nop k = k + 1), or n independent SALU instructions"""
    if n <= 0:
        return []
    return ["s_mov_b32 s90, %d" % k for k in range(n)] if filler else ["s_nop %d" % (n - 1)]


def cases():
    """function name -> (body lines, violation expected)"""
    out = {}
    for name, first, second, n in RULES:
        out[name + "_short"] = (first + pad(n - 1) + [second], True)
        out[name + "_exact"] = (first + pad(n) + [second], False)
        out[name + "_short_filler"] = (first + pad(n - 1, True) + [second], True)
        out[name + "_exact_filler"] = (first + pad(n, True) + [second], False)
    # state is kept across labels and comments, but not across the start of a function
    out["across_label_short"] = (["v_readfirstlane_b32 s4, v1", ".Lx:", "s_nop 3", "global_load_dword v2, v3, s[4:5]"], True)
    out["quoted_short"] = (QUOTED, True)
    out["quoted_fixed"] = (QUOTED_FIXED, False)
    out["a_new_function_starts_clean"] = (["v_xor_b32_e32 v4, s1, v4"], False)
    return out


def source(cs):
    lines = ["\t.text\n"]
    for k, (name, (body, _)) in enumerate(cs.items()):
        lines += ["\t.globl %s\n" % name, "\t.p2align 8\n", "\t.type %s,@function\n" % name, "%s:\n" % name]
        lines += [("%s\n" % b) if b.endswith(":") else "\t%s\n" % b for b in body]
        lines += ["\ts_endpgm\n", ".Lfunc_end%d:\n" % k, "\t.size %s, .Lfunc_end%d-%s\n" % (name, k, name)]
    return lines


@pytest.fixture(scope="module")
def assembled(tmp_path_factory):
    mc = os.path.join(A.LLVM, "llvm-mc")
    if not os.path.exists(mc):
        pytest.skip("no llvm-mc here")
    cs = cases()
    # the function that must start clean comes right behind one that ends with a write of s1: one wait state apart
    order = {k: v for k, v in cs.items() if k != "a_new_function_starts_clean"}
    order["ends_with_a_write"] = (["v_readlane_b32 s1, v127, 45"], False)
    order["a_new_function_starts_clean"] = cs["a_new_function_starts_clean"]
    d = tmp_path_factory.mktemp("isa")
    s = os.path.join(str(d), "cases.s")
    with open(s, "w") as f:
        f.writelines(source(order))
    o = os.path.join(str(d), "cases.o")
    subprocess.check_call([mc, "-arch=amdgcn", "-mcpu=gfx950", "-filetype=obj", s, "-o", o])
    return order, s, o


def flagged(path):
    funcs, _, bad = A.audit(path)
    return funcs, {v["function"] for v in bad}, bad


def test_each_rule_one_wait_state_short_is_flagged_and_exactly_padded_is_clean(assembled):
    cs, _, obj = assembled
    funcs, hit, bad = flagged(obj)
    assert set(funcs) == set(cs)
    want = {k for k, (_, v) in cs.items() if v}
    assert hit == want, ("missed", sorted(want - hit), "false alarms", sorted(hit - want))
    # one violation per flagged case, naming the writer and the reader
    assert len(bad) == len(want)
    for v in bad:
        body = cs[v["function"]][0]
        assert v["have"] < v["need"]
        assert v["first"] == body[0] and v["second"] in body[1:]


def test_the_quoted_site_across_an_asm_marker_pair(assembled):
    """the shipped sequence (readlane; s_nop 0; ;;#ASMSTART; ;;#ASMEND; v_xor) from the code object and from the text"""
    _, s, obj = assembled
    for path in (obj, s):
        _, hit, bad = flagged(path)
        assert "quoted_short" in hit and "quoted_fixed" not in hit, path
        v = [b for b in bad if b["function"] == "quoted_short"]
        assert len(v) == 1 and (v[0]["register"], v[0]["have"], v[0]["need"]) == ("s1", 1, 2)
        assert v[0]["first"] == "v_readlane_b32 s1, v127, 45" and v[0]["second"] == "v_xor_b32_e32 v4, s1, v4"


def test_text_and_object_give_the_same_verdicts(assembled):
    cs, s, obj = assembled
    f_s, hit_s, _ = flagged(s)
    f_o, hit_o, _ = flagged(obj)
    assert hit_s == hit_o
    # the object holds the instructions of the text, and an s_endpgm per function, nothing less
    for name, n in f_s.items():
        assert f_o[name] >= n, name


@built
def test_the_compilers_text_audits_clean():
    """calibration: the compiler pads what the hardware asks for, so a rule that flags its text is wrong"""
    funcs, kds, bad = A.audit(os.path.join(BUILD, "mcq_kernels.s"))
    assert kds is None and len(funcs) >= 31
    assert not bad, bad[:5]


@built
def test_the_code_object_inside_the_library_audits_clean_and_every_kernel_was_walked():
    funcs, kds, bad = A.audit(LIB)
    assert not bad, ["%s %s: %s / %s" % (v["function"], v["where"], v["first"], v["second"]) for v in bad[:10]]
    # every kernel descriptor has its function, and nothing else was walked
    assert kds and set(funcs) == kds, (sorted(set(funcs) ^ kds))
    assert len(kds) >= 31
    # a parser that sees nothing cannot pass: every kernel has real code, the evaluation kernels a lot of it
    for name, n in funcs.items():
        assert n >= 16, (name, n)
        if "mcq_eval_kernel" in name:
            assert n >= 4000, (name, n)
    assert sum(funcs.values()) >= 100000
    # the same code object as the build's own
    co = os.path.join(BUILD, "mcq_kernels.co")
    if os.path.exists(co):
        assert A.audit(co)[0] == funcs

"""CPU: the normaliser of tools/kernel_diff.py on hand-written listings (no compiler, no GPU).

Two links of the same kernel differ in instruction addresses and encodings, in the label a branch comment names, in the nop padding behind the
kernel and in the pc-relative offset of a named global: those must compare equal.  One changed instruction must not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_diff as KD  # noqa: E402

A = """\
0000000000007e00 <_Z4demoPf>:
	s_load_dwordx2 s[6:7], s[0:1], 0x18                        // 000000007E00: C0060180 00000018
	s_getpc_b64 s[8:9]                                         // 000000007E08: BE881C00
	s_add_u32 s8, s8, 0x45bc                                   // 000000007E0C: 8008FF08 000045BC
	s_addc_u32 s9, s9, 0                                       // 000000007E14: 8209FF09 00000000
	s_add_u32 s6, s6, 0x40                                     // 000000007E1C: 8006FF06 00000040
	s_cbranch_scc1 13                                          // 000000007E24: BF85000D <_Z4demoPf+0x58>
	v_add_f32_e32 v4, v4, v5                                   // 000000007E28: 02080B04
	s_endpgm                                                   // 000000007E2C: BF810000
	s_nop 0                                                    // 000000007E30: BF800000
	s_nop 0                                                    // 000000007E34: BF800000
"""
# the same kernel linked elsewhere: other addresses, other distance to the global, a label line, more padding
B = """\
0000000000019300 <_Z4demoPf>:
	s_load_dwordx2 s[6:7], s[0:1], 0x18                        // 000000019300: C0060180 00000018
	s_getpc_b64 s[8:9]                                         // 000000019308: BE881C00
	s_add_u32 s8, s8, 0x11c4                                   // 00000001930C: 8008FF08 000011C4
	s_addc_u32 s9, s9, 0                                       // 000000019314: 8209FF09 00000000
	s_add_u32 s6, s6, 0x40                                     // 00000001931C: 8006FF06 00000040
	s_cbranch_scc1 13                                          // 000000019324: BF85000D <L0>
<L0>:
	v_add_f32_e32 v4, v4, v5                                   // 000000019328: 02080B04
	s_endpgm                                                   // 00000001932C: BF810000
	s_nop 0                                                    // 000000019330: BF800000
	s_nop 0                                                    // 000000019334: BF800000
	s_nop 0                                                    // 000000019338: BF800000
		...
"""
C = B.replace("v_add_f32_e32 v4, v4, v5", "v_mul_f32_e32 v4, v4, v5")          # one instruction differs
D = B.replace("s_add_u32 s6, s6, 0x40 ", "s_add_u32 s6, s6, 0x80 ")            # an ordinary literal (not behind s_getpc) differs


def test_normaliser_drops_link_noise_and_keeps_instructions():
    a, b, c, d = (KD.disassembly(t)["_Z4demoPf"] for t in (A, B, C, D))
    assert a[0] == "s_load_dwordx2 s[6:7], s[0:1], 0x18" and a[-1] == "s_endpgm" and len(a) == 8
    assert a[2] == "s_add_u32 s8, s8, <pcrel>" and a[4] == "s_add_u32 s6, s6, 0x40"
    assert a == b                                                             # same
    assert a != c and [i for i, (x, y) in enumerate(zip(a, c)) if x != y] == [6]   # different: exactly the changed instruction
    assert a != d

"""csrc/control_wave_regd.inc is what tools/gen_wave_regd.py writes, and its DPP schedule keeps the distance the hardware asks
for: no v_*_dpp instruction reads an accumulator that one of the two instructions before it wrote, every statement opens
with `s_nop 1` (the compiler's own last instruction is then two issue slots away), and every element of D is taken exactly
once per pass from lane e % 16 of register e / 16."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_wave_regd as gen


def test_committed_file_is_the_generators_output():
    with open(gen.OUT) as f:
        assert f.read() == gen.render()


def statements(text):
    return [re.findall(r'"([^"]*)\\n\\t"', s) for s in re.findall(r"asm volatile\(\n(.*?)\n\s+:", text, flags=re.S) if "dpp" in s]


def test_schedule_keeps_two_slots_and_covers_D():
    for K in (5, 10):
        text, _, n_groups = gen.grad(K)
        stmts = statements(text)
        assert len(stmts) == n_groups
        seen = []
        for lines in stmts:
            assert lines[0] == "s_nop 1"
            slot, last = 0, {}
            for ln in lines:
                if ln.startswith("s_nop"):
                    slot += int(ln.split()[1]) + 1
                    continue
                m = re.match(r"v_(fmac_f64|mov_b64)_dpp %\[(\w+)\], %\[d(\d+)\](?:, %\[(\w+)\])? row_newbcast:(\d+) row_mask:0xf bank_mask:0xf$", ln)
                assert m, ln
                dst, q, lane = m.group(2), int(m.group(3)), int(m.group(5))
                assert slot - last.get(dst, -10) > 2, (K, ln)
                last[dst] = slot
                slot += 1
                seen.append((16 * q + lane, dst[0], m.group(1)))
        # G takes every element with k1 > 0 (row 0 by a move), h every element of the rows k2 > 0 (k1 = 0 by a move)
        want = [(e, "g", "mov_b64" if e < K else "fmac_f64") for e in range(K * K) if e % K > 0]
        want += [(e, "h", "mov_b64" if e % K == 0 else "fmac_f64") for e in range(K, K * K)]
        assert sorted(seen) == sorted(want)

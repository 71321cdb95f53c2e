#!/usr/bin/env python3
"""Writes ergodic_exploration_amd/csrc/control_wave_regd.inc: the gradient of the fp64 K = 5 / 10 wavefront kernel with
D = lambda (c - phi) in registers (csrc/control_wave_impl.hpp, kRegD).

Element e = k2 K + k1 of D lives in lane e % 16 of EVERY row of 16 lanes, register pair e / 16, and enters the
multiply-adds through the DPP row broadcast (v_fmac_f64_dpp row_newbcast:(e % 16)); where D enters without a product
(row k2 = 0 of G, h = D at k1 = 0) its bits are moved (v_mov_b64_dpp).  The arithmetic is that of the LDS form: G(k1)
accumulates over k2 = 1 .. K - 1 in order, one h chain per row in the order k1 = 0 .. K - 1.

A DPP instruction must not read a register -- its accumulator included -- that a vector instruction wrote in the two
issue slots before it.  The compiler does not keep that distance between one of its own instructions and an
inline-assembly statement, so the distance is part of the text: every statement opens with `s_nop 1` (whatever the
compiler wrote last is two slots away) and holds the DPP instructions of TWO rows -- rows 0 and 1, then pairs -- ordered
so that two instructions on one accumulator are at least two instructions apart: the two h chains and the G
accumulators fill each other's gaps, and only a last single row (K = 5: row 4) needs wait states of its own.  The
schedule is checked below before it is written.

    python tools/gen_wave_regd.py            # rewrite the file
    python tools/gen_wave_regd.py --check    # exit 1 if the committed file is not what this script writes
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "ergodic_exploration_amd", "csrc", "control_wave_regd.inc")
GAP = 2  # issue slots between a vector write of a register and a DPP read of it
DPP = "row_mask:0xf bank_mask:0xf"


def schedule(chains):
    """chains: lists of (dst, text) in program order per accumulator; returns lines with the wait states put in.
    Greedy: the ready chain with the most instructions left goes next."""
    pos = [0] * len(chains)
    last = {}   # dst -> slot of its last write
    slot, lines = 0, []
    total = sum(len(c) for c in chains)
    done = 0
    while done < total:
        ready = [i for i, c in enumerate(chains)
                 if pos[i] < len(c) and slot - last.get(c[pos[i]][0], -10) > GAP]
        if not ready:
            wait = min(last[c[pos[i]][0]] + GAP + 1 - slot for i, c in enumerate(chains) if pos[i] < len(c))
            lines.append(("s_nop %d" % (wait - 1), None))
            slot += wait
            continue
        i = max(ready, key=lambda i: (len(chains[i]) - pos[i], -i))
        dst, text = chains[i][pos[i]]
        lines.append((text, dst))
        last[dst] = slot
        pos[i] += 1
        slot += 1
        done += 1
    return lines


def check(lines):
    """no DPP instruction reads its accumulator within GAP slots of the instruction that wrote it"""
    slot, last = 0, {}
    for text, dst in lines:
        if dst is None:
            slot += int(text.split()[1]) + 1
            continue
        assert slot - last.get(dst, -10) > GAP, (text, lines)
        last[dst] = slot
        slot += 1


def statement(K, rows):
    """The DPP instructions of `rows` (row 0: the G moves) as one asm statement; returns (C++ text, wait states)."""
    nreg = (K * K + 15) // 16
    first = rows[0] == 0
    hrows = [r for r in rows if r > 0]
    qs = sorted({(r * K + i) // 16 for r in rows for i in range(K)})
    assert all(q < nreg for q in qs)
    gch = [[] for _ in range(K)]
    hch = []
    for r in rows:
        hn = "h%d" % hrows.index(r) if r > 0 else None
        h = []
        for i in range(K):
            e = r * K + i
            d, n = "d%d" % (e // 16), e % 16
            if r == 0:
                if i > 0:
                    gch[i].append(("g%d" % i, "v_mov_b64_dpp %%[g%d], %%[%s] row_newbcast:%d %s" % (i, d, n, DPP)))
                continue
            if i > 0:
                gch[i].append(("g%d" % i, "v_fmac_f64_dpp %%[g%d], %%[%s], %%[t%d] row_newbcast:%d %s"
                               % (i, d, hrows.index(r), n, DPP)))
            if i == 0:
                h.append((hn, "v_mov_b64_dpp %%[%s], %%[%s] row_newbcast:%d %s" % (hn, d, n, DPP)))
            else:
                h.append((hn, "v_fmac_f64_dpp %%[%s], %%[%s], %%[c%d] row_newbcast:%d %s" % (hn, d, i, n, DPP)))
        if h:
            hch.append(h)
    lines = [("s_nop 1", None)] + schedule(hch + [g for g in gch if g])
    check(lines)
    waits = sum(int(t.split()[1]) + 1 for t, d in lines[1:] if d is None)
    body = "\n".join('        "%s\\n\\t"' % t for t, _ in lines)
    outs = ['[g%d] "%s"(G[%d])' % (i, "=&v" if first else "+v", i) for i in range(1, K)]
    outs += ['[h%d] "=&v"(h%d)' % (n, n) for n in range(len(hrows))]
    ins = ['[d%d] "v"(Dv[%d])' % (q, q) for q in qs]
    ins += ['[t%d] "v"(t%d)' % (n, n) for n in range(len(hrows))]
    ins += ['[c%d] "v"(cxa[%d])' % (i, i) for i in range(1, K)]
    assert len(outs) + len(ins) <= 30
    text = "    asm volatile(\n%s\n        : %s\n        : %s);\n" % (body, ", ".join(outs), ", ".join(ins))
    return text, waits


def grad(K):
    nreg = (K * K + 15) // 16
    groups = [[0, 1]] + [[r, r + 1] for r in range(2, K - 1, 2)]
    if (K - 2) % 2:
        groups.append([K - 1])
    o = []
    o.append("template <>\nstruct RegDGrad<%d>\n{\n" % K)
    o.append("  static constexpr int kRegs = %d;\n" % nreg)
    o.append("  // G(k1) = sum_k2 D(k1,k2) cos(b_k2 y) for k1 = 1 .. %d; accy += sum_k2 k2 U_{k2-1}(cos b y) H(k2)\n" % (K - 1))
    o.append("  static __device__ __forceinline__ void run(const double (&Dv)[%d], const double (&cxa)[%d], double (&G)[%d],\n"
             "                                             double cy, double twoy, double& accy)\n  {\n" % (nreg, K, K))
    o.append("    double um = 0.0, u0 = 1.0;  // U_{k2-2}, U_{k2-1} of the y angle\n")
    o.append("    double tm = 1.0, t0 = cy;   // T_{k2-1}, T_{k2}\n")
    o.append("    double t1, h0, h1;\n")
    total = 0
    for g in groups:
        hrows = [r for r in g if r > 0]
        o.append("    // row%s %s\n" % ("s" if len(g) > 1 else "", ", ".join(str(r) for r in g)))
        if len(hrows) == 2:
            o.append("    t1 = twoy * t0 - tm;\n")
        text, waits = statement(K, g)
        total += waits
        o.append(text)
        if g[0] == 0:
            o.append("    G[0] = 0.0;  // (never used: k1 sin(0) = 0)\n")
        for n, r in enumerate(hrows):
            o.append("    accy = fma_k(u0 * h%d, %d, accy);\n" % (n, r))
            o.append("    {\n      const double un = twoy * u0 - um;\n      um = u0;\n      u0 = un;\n    }\n")
        if len(hrows) == 2:
            o.append("    tm = t1;\n    t0 = twoy * t1 - t0;\n")
        else:
            o.append("    {\n      const double tn = twoy * t0 - tm;\n      tm = t0;\n      t0 = tn;\n    }\n")
        o.append("    // (nothing else orders the rows: without this the y recurrences of all rows run ahead of the multiply-adds)\n"
                 '    asm volatile("" : "+v"(t0), "+v"(tm), "+v"(u0), "+v"(um));\n')
    o.append("    (void)t1;\n    (void)h1;\n  }\n};\n")
    return "".join(o), total, len(groups)


def render():
    o = ["// GENERATED by tools/gen_wave_regd.py (which says what this is and checks the schedule) -- do not edit.\n",
         "// Included by control_wave_impl.hpp inside namespace eea::wave.\n",
         "template <int K>\nstruct RegDGrad;\n"]
    for K in (5, 10):
        text, waits, n = grad(K)
        o.append("// K = %d: %d statements, %d wait states per step of a lane besides the %d that open the statements\n"
                 % (K, n, waits, 2 * n))
        o.append(text)
    return "".join(o)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv[1:]:
        with open(OUT) as f:
            sys.exit(0 if f.read() == text else 1)
    with open(OUT, "w") as f:
        f.write(text)

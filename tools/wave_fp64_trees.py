#!/usr/bin/env python3
"""The fp64 instructions of the wavefront control kernel's instances as expression trees, to compare two builds without a GPU
(profiles/wave_regd.txt section 1, profiles/wave_trim.txt): a change AROUND the arithmetic must leave every tree as it was --
which product of a two-product site is fused into the multiply-add is the compiler's choice by use counts, and code far from
the site can move it.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -mllvm -disable-machine-licm --cuda-device-only -S \
        csrc/control_wave_kernel.hip -o new.s          (likewise parent.s from the parent's sources)
    python tools/wave_fp64_trees.py parent.s new.s [--depth 3] [--only SUBSTRING]

Per kernel symbol: every instruction whose mnemonic names f64 is a node; its operands are the nodes that last wrote the
register pair in text order (copies by v_mov_b32 / v_mov_b64 are looked through), every other value is a leaf without identity,
scalar registers and constants are leaves by kind, and a value read from LDS is a leaf named by its immediate offset (what
tells cos from sin of the parked heading).  Products are commutative, and the sign of a v_mul is pulled out to its user.
Trees are cut at --depth levels, and the two builds' multisets of trees are compared; the exit status is the number of
kernels that differ.  Control flow is ignored (text order): equal code gives equal trees.  Where blocks moved, a register's
last writer in text order may be a block that does not run before the use: --blocks cuts the trees at basic-block labels
(no such noise, but a site whose operands come from another block loses their names) -- read both.
"""
import argparse
import collections
import re
import sys

LABEL = re.compile(r"^(_Z\w*control_wave_kernel\w*):")
VREG = re.compile(r"^(-?)(\|?)v(?:\[(\d+):(\d+)\]|(\d+))\|?$")


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = LABEL.match(line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
        elif s.startswith(".LBB") and s.endswith(":"):
            body.append("@label")
        elif s and not s.startswith(".") and not s.endswith(":"):
            body.append(s)
    return out


def parse_operand(tok):
    """(kind, neg, first register, registers)"""
    m = VREG.match(tok)
    if m:
        lo = int(m.group(3) if m.group(3) is not None else m.group(5))
        hi = int(m.group(4)) if m.group(4) is not None else lo
        return "v", m.group(1) == "-", lo, hi - lo + 1
    neg = tok.startswith("-") and not re.match(r"^-[\d.]", tok)
    t = tok.lstrip("-").strip("|")
    if re.match(r"^(s\d+|s\[\d+:\d+\]|vcc|exec|ttmp)", t):
        return "s", neg, 0, 0
    if re.match(r"^a(\d+|\[)", t):
        return "a", neg, 0, 0
    return "c:" + tok, False, 0, 0


class Node(object):
    __slots__ = ("op", "srcs", "memo")

    def __init__(self, op, srcs):
        self.op, self.srcs, self.memo = op, srcs, {}


def pulled_sign(node):
    """the sign a v_mul hands to its user, also where the tree is cut"""
    if node is None or not node.op.startswith("v_mul_f64"):
        return False
    if "sign" not in node.memo:
        node.memo["sign"] = False  # (no cycles in straight-line text; a guard all the same)
        s = False
        for kind, neg, child in node.srcs:
            s ^= neg ^ (pulled_sign(child) if kind == "v" else False)
        node.memo["sign"] = s
    return node.memo["sign"]


def tree(node, depth):
    """(sign pulled out, text)"""
    if node is None:
        return False, "L"
    if node.op.startswith("lds:"):
        return False, node.op
    if depth == 0:
        return pulled_sign(node), "N"
    if depth in node.memo:
        return node.memo[depth]
    subs = []
    for kind, neg, child in node.srcs:
        if kind == "v":
            s, t = tree(child, depth - 1)
            subs.append((neg ^ s, t))
        else:
            subs.append((neg, kind))
    op = node.op
    if op.startswith("v_mul_f64"):
        r = (subs[0][0] ^ subs[1][0], "mul(%s)" % ",".join(sorted(t for _, t in subs)))
    elif op.startswith("v_fma_f64") or op.startswith("v_fmac_f64") or op.startswith("v_mfma_f64"):
        prod = sorted(t for _, t in subs[:2])
        ps = subs[0][0] ^ subs[1][0]
        r = (False, "%s(%s%s*%s,%s%s)" % ("mfma" if "mfma" in op else "fma", "-" if ps else "", prod[0], prod[1],
                                          "-" if subs[2][0] else "", subs[2][1]))
    else:
        args = ["%s%s" % ("-" if s else "", t) for s, t in subs]
        if op.startswith(("v_add_f64", "v_max_f64", "v_min_f64")):
            args.sort()
        r = (False, "%s(%s)" % (re.sub(r"_e32|_e64|_dpp", "", op), ",".join(args)))
    node.memo[depth] = r
    return r


def trees_of(body, depth, blocks=False):
    last = {}  # 32-bit vector register -> Node or None
    lds = {}
    nodes = []
    for s in body:
        if s == "@label":
            if blocks:  # values from another basic block are leaves
                last = {}
            continue
        parts = s.split(None, 1)
        op = parts[0]
        toks = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
        toks = [t.split()[0] for t in toks if t]  # drop modifiers behind an operand
        if not toks:
            continue
        dst = parse_operand(toks[0])
        if "_f64" in op and op.startswith("v_") and not op.startswith("v_cmp"):
            srcs = []
            for t in toks[1:4]:
                kind, neg, lo, n = parse_operand(t)
                if kind == "v":
                    a, b = last.get(lo), last.get(lo + 1) if n > 1 else last.get(lo)
                    srcs.append(("v", neg, a if a is b else None))
                elif kind in ("s", "a") or kind.startswith("c:"):
                    if not re.match(r"^c:(row_|quad_|bank_|bound_|op_sel|cbsz|abid|blgp|neg_|clamp|mul:|div:)", kind):
                        srcs.append((kind, neg, None))
            if op.startswith("v_fmac_f64") and dst[0] == "v":
                a, b = last.get(dst[2]), last.get(dst[2] + 1)
                srcs = srcs[:2] + [("v", False, a if a is b else None)]
            node = Node(op, srcs)
            nodes.append(node)
            if dst[0] == "v":
                for r in range(dst[2], dst[2] + max(dst[3], 1)):
                    last[r] = node
        elif op.startswith("ds_read") and dst[0] == "v":
            # a value read from LDS is a leaf WITH identity: its immediate offset (the kernel's LDS layout is fixed)
            offs = [int(x, 0) for x in re.findall(r"offset[01]?:(0x[0-9a-fA-F]+|\d+)", s)]
            unit = 512 if "2st64" in op else 8
            if op.startswith("ds_read2") and len(offs) < 2:
                offs = ([0] + offs) if "offset1" in s else (offs + [0]) if offs else [0, 0]
            for i in range(max(dst[3], 1)):
                if op.startswith("ds_read2"):
                    off = offs[i // 2] * unit
                else:
                    off = (offs[0] if offs else 0) + 8 * (i // 2)
                key = (dst[2] + i - i % 2, off)
                last[dst[2] + i] = lds.setdefault(key, Node("lds:%d" % off, []))
        elif op in ("v_mov_b32_e32", "v_mov_b64_e32") and dst[0] == "v":
            src = parse_operand(toks[1])
            for i in range(dst[3]):
                last[dst[2] + i] = last.get(src[2] + i) if src[0] == "v" else None
        elif dst[0] == "v" and not op.startswith(("global_store", "ds_write", "buffer_store", "scratch_store", "flat_store",
                                                  "v_cmp", "s_")):
            for r in range(dst[2], dst[2] + max(dst[3], 1)):
                last[r] = None
            if op.startswith("v_permlane32_swap") or op.startswith("v_swap"):
                o = parse_operand(toks[1])
                if o[0] == "v":
                    last[o[2]] = None
    return collections.Counter(tree(n, depth)[1] for n in nodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--only", default="Id", help="kernel symbols that contain this (default: the fp64 instances)")
    ap.add_argument("--blocks", action="store_true",
                    help="cut the trees at basic-block labels too: a register whose last writer in text order sits in a block "
                         "that does not run before the use (a loop's tail placed early) gives trees that differ for no reason")
    ap.add_argument("--show", type=int, default=12, help="differing trees printed per kernel")
    a = ap.parse_args()
    kp, kn = kernels(a.parent), kernels(a.new)
    differ = 0
    for name in sorted(kp):
        if a.only not in name:
            continue
        if name not in kn:
            print("%s: not in %s" % (name, a.new))
            differ += 1
            continue
        tp, tn = trees_of(kp[name], a.depth, a.blocks), trees_of(kn[name], a.depth, a.blocks)
        gone, come = tp - tn, tn - tp
        tag = re.search(r"kernelI(\w+?)EEv", name).group(1)
        print("%-40s fp64 instructions %5d -> %5d   trees only in parent %4d, only in new %4d" %
              (tag, sum(tp.values()), sum(tn.values()), sum(gone.values()), sum(come.values())))
        if gone or come:
            differ += 1
            for sign, c in (("-", gone), ("+", come)):
                for t, n in c.most_common(a.show):
                    print("    %s %3d x %s" % (sign, n, t))
    return differ


if __name__ == "__main__":
    sys.exit(min(main(), 255))

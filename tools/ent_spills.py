#!/usr/bin/env python3
"""Static instructions and SGPR spill / reload instructions per source region of an entropy kernel.

Input: the `hipcc -S -gline-tables-only` assembly of k_entropy.hip or of one of its builds (k_entropy_c.hip, ...).  Every instruction is
attributed to the source line of its .loc (the innermost inlined callee, as tools/isa_lines.py does), and the line to a region of
k_entropy.hip: the regions are named by the `// @region <name>` lines of that file, each running to the next one.  The compiler spills
scalar registers into the lanes of a VGPR that it names itself in the assembly ("SGPR spill to VGPR lane"); a spill is a v_writelane_b32
to that register, a reload a v_readlane_b32 from it.  Instructions without a source line (`.loc` with line 0) are counted in a row of their own.

Usage: ent_spills.py file.s [k_entropy.hip]
   or: hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S -gline-tables-only k_entropy_c.hip -o - | ent_spills.py -"""
import collections
import os
import re
import sys

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h264decode_amd", "csrc", "k_entropy.hip")
# `.loc <file> 0`: an instruction the compiler gives no line (block glue, loop exits, merged code).  It belongs to no region of the source -- least of all to
# 'other', the lines in front of the first marker -- and gets a row of its own, behind the regions.
NO_LINE = "(no source line)"
_INSN = re.compile(r"\s+((?:[sv]|ds|global|buffer|flat|scratch)_[a-z0-9_]+)\s*(.*)")


def regions(source=SOURCE):
    """[(first_line, name)] in file order, from the `// @region` lines; lines in front of the first one belong to 'other'."""
    out = [(1, "other")]
    for no, line in enumerate(open(source), 1):
        m = re.match(r"// @region (.+?)\s*$", line)
        if m:
            out.append((no, m.group(1)))
    return out


def region_of(line_no, regs):
    name = regs[0][1]
    for first, n in regs:
        if first > line_no:
            break
        name = n
    return name


def spill_vgprs(asm_text):
    """The VGPRs the compiler keeps spilled SGPRs in, from its own notes."""
    return sorted(set(re.findall(r"\$(vgpr\d+)\s*:\s*SGPR spill to VGPR lane", asm_text)))


def table(asm_text, source=SOURCE):
    """{region: Counter(insts, spills, reloads)}, the names of the spill VGPRs, and the instructions that belong to no line of `source`."""
    regs = regions(source)
    src_name = os.path.basename(source)
    files = {int(n): (f if not d else d + "/" + f) for n, d, f in re.findall(r'^\s*\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', asm_text, re.M)}
    ours = {n for n, f in files.items() if os.path.basename(f) == src_name}
    sv = ["v" + v[4:] for v in spill_vgprs(asm_text)]
    out = collections.OrderedDict((n, collections.Counter()) for _, n in regs)
    out[NO_LINE] = collections.Counter()
    foreign = 0
    cur = None
    for line in asm_text.splitlines():
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2)))
            continue
        m = _INSN.match(line)
        if not m or cur is None:
            continue
        if cur[0] not in ours:
            foreign += 1
            continue
        c = out[region_of(cur[1], regs) if cur[1] else NO_LINE]
        c["insts"] += 1
        op, args = m.group(1), [a.strip() for a in m.group(2).split(";")[0].split(",")]
        if op == "v_writelane_b32" and args[0] in sv:
            c["spills"] += 1
        elif op == "v_readlane_b32" and len(args) > 1 and args[1] in sv:
            c["reloads"] += 1
    return out, sv, foreign


def render(asm_text, source=SOURCE):
    tab, sv, foreign = table(asm_text, source)
    lines = ["spill VGPRs: %s" % (", ".join(sv) or "none"), "%-30s %8s %8s %8s" % ("region", "insts", "spills", "reloads")]
    tot = collections.Counter()
    for name, c in tab.items():
        if not c["insts"]:
            continue
        tot.update(c)
        lines.append("%-30s %8d %8d %8d" % (name, c["insts"], c["spills"], c["reloads"]))
    lines.append("%-30s %8d %8d %8d" % ("total", tot["insts"], tot["spills"], tot["reloads"]))
    if foreign:
        lines.append("(%d instructions of other files, headers, are not counted)" % foreign)
    for key in ("sgpr_spill_count", "vgpr_count", "private_segment_fixed_size"):
        m = re.search(r"\.%s:\s+(\d+)" % key, asm_text)
        if m:
            lines.append("%s: %s" % (key, m.group(1)))
    m = re.search(r"codeLenInByte = (\d+)", asm_text)
    if m:
        lines.append("codeLenInByte: %s" % m.group(1))
    return "\n".join(lines)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    text = sys.stdin.read() if sys.argv[1] == "-" else open(sys.argv[1]).read()
    print(render(text, sys.argv[2] if len(sys.argv) > 2 else SOURCE))

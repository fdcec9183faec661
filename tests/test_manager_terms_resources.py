"""Code-object budget of zb_m_terms_step_kernel<kTgs, kOcc>, read from the built libzbot.so as
tests/test_kernel_resources.py reads it (no GPU needed). The build keeps the manager kernels' budget:
kOcc = 2 at most 256 VGPR + AGPR, 64 B of scratch per lane and 20 KB of LDS; kOcc = 1 no scratch at all.
Its scratch accesses inside loops are held to those of the dr build (zb_m_dr_step_kernel, the same text
without the five reward terms) with the same template arguments. Three of the four builds have no more
than the dr build. The TGS build at two waves per SIMD has one more: of the three per-lane 64-bit
broadphase masks that the prologue forms, the dr build parks two in scratch and reloads them inside the
detection loops, and the terms build parks all three (4 in-loop reloads against 3; 56 B of scratch
against 52 B). That figure is accepted and asserted here as it stands, so that it cannot grow unseen;
no build stores to scratch inside a loop."""
import re

import test_kernel_resources as K

TERMS, DR = "22zb_m_terms_step_kernel", "19zb_m_dr_step_kernel"


def test_terms_step_kernel_budget(tmp_path):
    found = 0
    for name, md in K._kernel_metadata(tmp_path).items():
        if TERMS not in name:
            continue
        found += 1
        occ = int(re.search(r"ILb[01]ELi([12])EE", name).group(1))
        regs, lds, scratch = md["vgpr_count"], md["group_segment_fixed_size"], md.get("private_segment_fixed_size", 0)
        print(f"{name[18:51]}: {regs} regs, {lds} B LDS, {scratch} B scratch")
        assert lds <= 20 * 1024
        if occ == 1:
            assert regs <= 512 and scratch == 0, (name, regs, scratch)
        else:
            assert regs <= 256 and scratch <= 64, (name, regs, scratch)
    assert found == 4


def _in_loop_scratch(text):
    """{kernel symbol: (scratch instructions inside a loop, all scratch instructions, loops, scratch stores
    inside a loop)} of the terms and dr builds; a loop is the span between a backward branch and its target."""
    out, cur, base, insts, brs = {}, None, 0, [], []

    def close():
        if cur is not None:
            loops = [(d, s) for s, d in brs if d <= s]
            scr = [a for a, ins in insts if ins.startswith("scratch_")]
            st = [a for a, ins in insts if ins.startswith("scratch_store")]
            inside = lambda xs: sum(1 for a in xs if any(d <= a <= s for d, s in loops))
            out[cur] = (inside(scr), len(scr), len(loops), inside(st))

    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            close()
            cur = m.group(2) if (TERMS in m.group(2) or DR in m.group(2)) else None
            base, insts, brs = int(m.group(1), 16), [], []
            continue
        if cur is None:
            continue
        a = re.search(r"// ([0-9A-F]{6,}):", line)
        if not a:
            continue
        addr, ins = int(a.group(1), 16), line.split("//")[0].strip()
        insts.append((addr, ins))
        t = re.search(r"<\S+\+0x([0-9a-f]+)>", line)
        if re.match(r"s_(cbranch_\w+|branch) ", ins) and t:
            brs.append((addr, base + int(t.group(1), 16)))
    close()
    return out


def test_terms_step_kernel_in_loop_scratch(tmp_path):
    res = _in_loop_scratch(K._disassembly(tmp_path))
    checked = 0
    for name, (inside, total, loops, stores) in sorted(res.items()):
        if TERMS not in name:
            continue
        targs = re.search(r"(ILb[01]ELi[12]EE)", name).group(1)
        dr = [v for k, v in res.items() if DR in k and targs in k]
        assert len(dr) == 1 and loops > 0 and dr[0][2] > 0, name
        print(f"{name[18:51]}: {inside} of {total} scratch instructions inside loops (dr build: {dr[0][0]} of {dr[0][1]})")
        extra = 1 if targs == "ILb1ELi2EE" else 0  # (TGS, two waves per SIMD: the third broadphase mask)
        assert stores == 0, f"{name[:52]}: {stores} scratch stores inside loops"
        assert inside <= dr[0][0] + extra, f"{name[:52]}: {inside} scratch accesses inside loops, the dr build has {dr[0][0]}"
        checked += 1
    assert checked == 4

"""CPU tests (cross-compiled assembly, no GPU) of how the fp64 sum-product kernels treat their arguments and their scalar registers
(profiles/NOTES.md R8.1): what only the epilogue needs is read from the kernel-argument segment behind the iteration loop, nothing scalar is
kept in the lanes of a vector register inside that loop, and the steady-state bin loop holds fewer scalar instructions than the parent's."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["mgpu_ldpc_spa_kernel_ne%d" % ne for ne in (4, 5, 6, 7, 8)]

# Measured on the parent commit with the same counting rule as tests/test_abi.py (instructions starting with s_ in the blocks of the largest
# depth-2 loop, s_waitcnt and s_nop left out): tools/isa_count.py's compile of the parent's ldpc.hip, kernel ne6.
PARENT_STEADY_SALU_NE6 = 162
PARENT_LANE_SPILL_OPS_NE6 = 241       # v_readlane_b32 + v_writelane_b32 in the whole kernel (parent); for the record


@pytest.fixture(scope="module")
def asm():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_count
    return isa_count.assembly("ldpc.hip")


def _body(lines, kern):
    start = next(i for i, l in enumerate(lines) if l.startswith(kern + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return start, end


def _is_insn(t):
    return bool(t) and t[0] not in ";." and not t.endswith(":")


def _iteration_loop(lines, start, end):
    """(instructions inside the iteration loop, line index of its header, line index of its last block's end). The iteration loop is the
    depth-1 loop with depth-2 children (the two copies of the bin loop)."""
    header = None
    for i in range(start, end):
        if "Loop Header: Depth=1" in lines[i] and "Child Loop" in lines[i + 1]:
            assert header is None, "more than one depth-1 loop with children"
            header = i
    assert header is not None
    name = lines[header].split(":")[0][2:]                   # ".LBB2_52" -> "BB2_52", as the block annotations spell it
    children = set()
    j = header + 1
    while "Child Loop" in lines[j]:
        children.add(re.search(r"Child Loop (BB\d+_\d+)", lines[j]).group(1))
        j += 1
    assert len(children) == 2, children
    inside, insns, last = False, [], header
    for i in range(header, end):
        l = lines[i]
        if re.match(r"^\.LBB\d+_\d+:", l) or l.startswith("; %bb."):
            label = l.split(":")[0][2:]
            m = re.search(r"Header=(BB\d+_\d+) Depth=(\d)", l)
            inside = i == header or label in children or (m is not None and (m.group(1) == name or m.group(1) in children))
            continue
        t = l.strip()
        if inside and _is_insn(t):
            insns.append(t)
            last = i
    return insns, header, last


# v_readlane_b32 + v_writelane_b32 inside the iteration loop, measured on the parent commit (same rule as below): the bar for rate 14/16
PARENT_LANE_OPS_IN_ITERATION_LOOP = {"mgpu_ldpc_spa_kernel_ne4": 80, "mgpu_ldpc_spa_kernel_ne5": 88, "mgpu_ldpc_spa_kernel_ne6": 96,
                                     "mgpu_ldpc_spa_kernel_ne7": 104, "mgpu_ldpc_spa_kernel_ne8": 84}


@pytest.mark.parametrize("kern", KERNELS)
def test_no_scalar_lives_in_vector_lanes_inside_the_iteration_loop(asm, kern):
    """Rates 1/16 ... 8/16 (ne4 ... ne7): no lane read or write of a spilled scalar anywhere inside the iteration loop. Rate 14/16 (ne8) requests
    all eight rounds' lane masks at once in the look before the first iteration (ldpc.hip: syn_judge - a launch of hard frames is that look, and
    the modes that deliver hard frames use this rate), which leaves its allocator one scalar to keep in a lane around each bin loop: there the
    bar is none inside the bin loops themselves (what is paid per bin) and, per iteration, strictly fewer than the parent's measured count."""
    start, end = _body(asm, kern)
    insns, header, last = _iteration_loop(asm, start, end)
    assert len(insns) > 1000, len(insns)                     # both bin loops and what stands between them were found
    lane_ops = [t for t in insns if t.startswith(("v_readlane_b32", "v_writelane_b32"))]
    print(kern, "lane operations inside the iteration loop:", len(lane_ops), "parent", PARENT_LANE_OPS_IN_ITERATION_LOOP[kern])
    if not kern.endswith("ne8"):
        assert not lane_ops, (kern, lane_ops)
        return
    assert len(lane_ops) < PARENT_LANE_OPS_IN_ITERATION_LOOP[kern], (kern, lane_ops)
    in_bin_loops, inside = [], False
    for l in asm[header:last + 1]:
        if re.match(r"^\.LBB\d+_\d+:", l) or l.startswith("; %bb."):
            inside = "Depth=2" in l or "Parent Loop" in l
            continue
        if inside and l.strip().startswith(("v_readlane_b32", "v_writelane_b32")):
            in_bin_loops.append(l.strip())
    assert not in_bin_loops, (kern, in_bin_loops)


@pytest.mark.parametrize("kern", KERNELS)
def test_registers_scratch_and_static_lds(asm, kern):
    start, end = _body(asm, kern)
    foot = "\n".join(asm[end:end + 200])
    assert int(re.search(r"; NumVgprs: (\d+)", foot).group(1)) <= 64, kern
    assert int(re.search(r"; ScratchSize: (\d+)", foot).group(1)) == 0, kern
    assert int(re.search(r"; Occupancy: (\d+)", foot).group(1)) == 8, kern
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", "\n".join(asm[start:end + 200])).group(1)) == 0, kern       # the kernel traps unless its dynamic LDS block starts at address 0
    assert not any("scratch_" in l for l in asm[start:end]), kern


def test_steady_state_bin_loop_holds_fewer_scalar_instructions_than_the_parent(asm):
    start, end = _body(asm, "mgpu_ldpc_spa_kernel_ne6")
    loops, key = {}, None
    for l in asm[start:end]:
        if re.match(r"^\.LBB\d+_\d+:", l) or l.startswith("; %bb."):
            m = re.search(r"Header=(BB\d+_\d+) Depth=2", l)
            key = m.group(1) if m else None
            continue
        t = l.strip()
        if key and t and t[0] not in ";.":
            loops.setdefault(key, []).append(t)
    steady = max(loops.values(), key=len)
    salu = sum(1 for t in steady if t.startswith("s_") and not t.startswith(("s_waitcnt", "s_nop")))
    print("steady-state scalar instructions: %d (parent %d)" % (salu, PARENT_STEADY_SALU_NE6))
    assert salu < PARENT_STEADY_SALU_NE6, salu
    # the address table's descriptor stays one four-register value across the bin loop: the buffer load at a bin's end is not preceded by moves
    # that re-form its constant words
    loads = [i for i, t in enumerate(steady) if t.startswith("buffer_load_dwordx2")]
    assert len(loads) == 1, loads
    assert not [t for t in steady[loads[0] - 4:loads[0]] if t.startswith("s_mov_b32")], steady[loads[0] - 4:loads[0] + 1]


def _kernel_args(asm, kern):
    """(offset, size, kind) of the kernel's arguments from the code object's metadata."""
    name = next(i for i, l in enumerate(asm) if re.match(r"^\s+\.name:\s+%s$" % kern, l))
    top = max(i for i in range(name) if asm[i].strip() == ".args:")
    args, cur = [], {}
    for l in asm[top + 1:name]:
        m = re.match(r"^\s+(- )?\.(\w+):\s+(\S+)", l)
        if not m or (not m.group(1) and not l.startswith("        ")):
            break
        if m.group(1) and cur:
            args.append(cur)
            cur = {}
        cur[m.group(2)] = m.group(3)
    args.append(cur)
    return [(int(a["offset"]), int(a["size"]), a["value_kind"]) for a in args if "offset" in a]


@pytest.mark.parametrize("kern", KERNELS)
def test_argument_segment_is_laid_out_as_the_late_reads_assume(asm, kern):
    """ldpc.hip: SpaKernArgs restates the argument segment (the tables by value, then eight arguments at their natural alignment) and pins
    it on the structs with static_asserts; this pins the restatement on what the compiler laid out, and the late reads on where they stand:
    no load of an output / variance pointer or of the tail's tables and sizes in front of the iteration loop's end, all of them behind it,
    judged on the loads whose base register is the segment pointer (the hard-frame counters' address is used in front of the loop only and
    stays a parameter)."""
    args = [a for a in _kernel_args(asm, kern) if not a[2].startswith("hidden_")]
    assert len(args) == 9 and args[0][0] == 0 and args[0][2] == "by_value", args
    T = args[0][1]
    assert T % 8 == 0
    assert [a[0] for a in args[1:]] == [T + 8 * k for k in range(8)], args
    assert [a[1] for a in args[1:]] == [8, 4, 8, 8, 8, 8, 8, 8], args
    start, end = _body(asm, kern)
    _, header, last = _iteration_loop(asm, start, end)
    # what only the epilogue reads, as byte ranges of the segment: LdpcDev's scrambler, crc_tab, crc_init (16..36), K (120..124), nReal and
    # payload_stride (128..136) - device_tables.h, 160 bytes; a change of that struct has to restate these - and the six pointers behind F
    assert T == 160, "LdpcDev changed: restate the epilogue's fields below"
    late = [(16, 36), (120, 124), (128, 136), (T + 16, T + 64)]
    loads = _kernarg_loads(asm, start, end)
    assert loads, "no load from the argument segment recognised"
    assert all(hi is not None for _, lo, hi in loads), [asm[i].strip() for i, lo, hi in loads if hi is None]      # (an offset register: cannot be judged)

    def touching(first, past):
        return [(asm[i].strip(), r) for i, lo, hi in loads if first <= i < past for r in late if lo < r[1] and hi > r[0]]
    assert [i for i, lo, hi in loads if i < header], "the entry's own argument loads were not recognised"
    assert not touching(start, header), (kern, touching(start, header))                   # nothing of it in front of the iteration loop
    behind = touching(last + 1, end)
    assert {r for _, r in behind} == set(late), (kern, behind)                            # all of it behind the loop, through the segment pointer


def _sregs(tok):
    m = re.match(r"^s\[(\d+):(\d+)\]$", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^s(\d+)$", tok)
    return [int(m.group(1))] if m else []


def _kernarg_loads(asm, start, end):
    """(line index, first byte, byte past the end) of every scalar load in the kernel whose BASE is the kernel-argument segment pointer: the
    pair s[0:1] at entry (the kernels' only user scalars), any pair it is copied to by s_mov_b64, and a pair restored from the vector lanes
    it was written to - for as long as the pair holds nothing else. A load with an offset register has None for its end."""
    bases, lanes, restored, out = {(0, 1)}, {}, {}, []
    for i in range(start, end):
        t = asm[i].strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op, _, rest = t.partition(" ")
        ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", rest)] if rest else []
        if op.startswith("s_load_dword"):
            base = tuple(_sregs(ops[1]))
            if base in bases:
                n = int(op[len("s_load_dword"):].lstrip("x") or 1)
                m = re.match(r"^(0x[0-9a-f]+|\d+)$", ops[2]) if len(ops) == 3 else None
                off = int(m.group(1), 0) if m else None
                out.append((i, off if m else 0, off + 4 * n if m else None))
        if op == "v_writelane_b32":
            for b in bases:
                if _sregs(ops[1]) and _sregs(ops[1])[0] in b:
                    lanes[(ops[0], ops[2])] = b.index(_sregs(ops[1])[0])
            continue
        if op.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_barrier", "v_", "ds_", "buffer_", "global_")) and op != "v_readlane_b32" and op != "v_readfirstlane_b32":
            if not op.startswith("v_cmp"):
                continue
        dest = set(_sregs(ops[0])) if ops else set()
        if op.startswith(("s_and_saveexec", "s_andn2_saveexec", "s_or_saveexec")) or op.startswith("v_cmp"):
            dest = set(_sregs(ops[0]))
        copied = op == "s_mov_b64" and tuple(_sregs(ops[1])) in bases
        half = lanes.get((ops[1], ops[2])) if op == "v_readlane_b32" else None
        bases = {b for b in bases if not dest & set(b)}
        restored = {r: h for r, h in restored.items() if r not in dest}
        if copied:
            bases.add(tuple(_sregs(ops[0])))
        if half is not None:
            r = _sregs(ops[0])[0]
            restored[r] = half
            for lo in (r, r - 1):
                if restored.get(lo) == 0 and restored.get(lo + 1) == 1:
                    bases.add((lo, lo + 1))
    return out

"""Instruction counts along the paths a wave takes through the INTERIOR-STEP loop of a fill kernel's ISA.

    python tools/isa_hot_path.py [--dump] k.s [kernel-name-substring] [top-N]

k.s is hipcc's -S output (--cuda-device-only) of a translation unit; the kernel is the first one whose symbol contains
the substring (default: fill_affine_slim_kernelILi1ELi3ELi4ELb0E, the headline's).  The interior-step loop is a depth-2
loop of that kernel with at least 100 vector instructions (the others are the spin loops of the team hand-off); where the
boundary steps form a depth-2 loop of their own (fill_affine_slim_kernel) it is the one with fewer of them.

Two kinds of path from the loop header back to it are printed:
  * the per-step hot path: no ghost-block boundary work (no counted vmcnt wait, no DMA), no rare work;
  * the block-boundary path: through wait_block, the in-place unpack of the landed block and the DMAs of the next one.
    Where the loop holds the steady form of the DMAs (scalar base: `global_load_lds_dwordx4 v, s[..]`), the path through
    it is printed first, then the one through the general form (`global_load_lds_dwordx4 v[..], off`).
A path avoids rare work (error flag, partner wait).  At a branch both ways are tried -- into the guarded block of an
exec-mask skip first (some lane is active as a rule), else fall-through first (the hot path: also the taken way of scalar
branches first, and the shorter of the two paths) -- and the first complete path counts:
of wait_block's ladder it takes one rung, and it may include the few instructions of the range check that runs every
16 steps.
For a boundary path the script also prints its two sections: the unpack (first ds_read_b128 .. last ds_write_b128) and
the DMA section (what follows the unpack up to the last DMA's m0 restore), and every 64-bit / full multiply on the path.

    python tools/isa_hot_path.py --traceback k.s [kernel-name-substring] [top-N]

Traceback mode: the column loop of an affine traceback kernel (default: traceback_affine_fast_kernelILi1E; the generic
one is traceback_affine_kernelILi1ELb1ELb0ELb0ELb1ELb0ELb0E, whose loop is walk_affine's, inlined) is the depth-1 loop that
holds the pick's v_readlane.  One
path is printed, the common one of a column: through the candidates' global loads and the pick, with no 64-bit multiply-add
where the loop has a path without one (the short-chain kernel's side path through full records divides and multiplies in
64 bits; the generic kernel does so in every column) and without the trace buffer's flush."""
import collections, re, sys

sys.setrecursionlimit(100000)
TRACEBACK = "--traceback" in sys.argv
if TRACEBACK:
    sys.argv.remove("--traceback")
DUMP = "--dump" in sys.argv  # also list the instructions of the per-step hot path, in order
if DUMP:
    sys.argv.remove("--dump")
src = open(sys.argv[1]).read().split("\n")
want = sys.argv[2] if len(sys.argv) > 2 else ("traceback_affine_fast_kernelILi1E" if TRACEBACK else "fill_affine_slim_kernelILi1ELi3ELi4ELb0E")
top = int(sys.argv[3]) if len(sys.argv) > 3 else 14

start = next((i for i, l in enumerate(src) if re.match(r"^_Z\w+:", l) and want in l), None)
if start is None:
    sys.exit(f"no kernel matching {want!r} in {sys.argv[1]}")
end = next(i for i in range(start, len(src)) if src[i].strip().startswith("s_endpgm"))
print("kernel:", src[start].rstrip(":"))

# ---- basic blocks: a block starts at a label, at a "; %bb.N:" note, or after a branch
Block = collections.namedtuple("Block", "name loop ops succ")
blocks, order = {}, []
cur = None


def open_block(name, loop):
    global cur
    cur = Block(name, loop, [], [])
    blocks[name] = cur
    order.append(name)


open_block("entry", None)
anon = 0
for l in src[start + 1:end + 1]:
    m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
    b = re.match(r"^; %bb\.(\d+):(.*)", l)
    if m or b:
        note = (m or b).group(2)
        name = m.group(1) if m else "%bb." + b.group(1)
        h = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", note)
        loop = (h.group(1), int(h.group(2))) if h else ("?" if "Loop" in note else None)
        prev = cur
        if prev.ops or prev.name == "entry" or m:
            open_block(name, loop)
            if not (prev.ops and prev.ops[-1].split()[0] == "s_branch"):
                prev.succ.append(name)
        else:  # a note right after a branch opened an anonymous block: name it
            cur = cur._replace(loop=loop)
            blocks[cur.name] = cur
        continue
    t = l.strip()
    if not t or t[0] in ";." or t.startswith("//"):
        continue
    if cur.loop == "?":  # a loop header's own lines ("Parent Loop", "This Loop Header") carry no Header= note
        pass
    cur.ops.append(t)
    op = t.split()[0]
    if op == "s_branch" or op.startswith("s_cbranch"):
        prev = cur
        anon += 1
        open_block(f"anon{anon}", prev.loop)
        prev.succ.append(t.split()[1])
        if op != "s_branch":
            prev.succ.append(cur.name)

# a loop header's label line says "This (Inner) Loop Header: Depth=d" instead of "Header=": resolve from the source
hdr_depth = {}
for i in range(start, end):
    m = re.match(r"^(\.LBB\d+_\d+):", src[i])
    if m:
        for j in range(i, min(i + 4, end)):
            d = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", src[j])
            if d:
                hdr_depth[m.group(1)[2:]] = int(d.group(1))
            if j > i and not src[j].lstrip().startswith(";"):
                break
for name in order:
    if blocks[name].loop == "?" and name[2:] in hdr_depth:
        blocks[name] = blocks[name]._replace(loop=(name[2:], hdr_depth[name[2:]]))

valu = lambda ops: sum(1 for o in ops if o.startswith("v_"))
DEPTH = 1 if TRACEBACK else 2
per_loop = collections.Counter()
for name in order:
    b = blocks[name]
    if isinstance(b.loop, tuple) and b.loop[1] == DEPTH:
        per_loop[b.loop[0]] += valu(b.ops)
if TRACEBACK:  # the column loop: the one with the pick
    picks = {blocks[n].loop[0] for n in order if isinstance(blocks[n].loop, tuple) and blocks[n].loop[1] == 1 and
             any(o.startswith("v_readlane") for o in blocks[n].ops)}
    per_loop = collections.Counter({k: v for k, v in per_loop.items() if k in picks})
if not per_loop:
    sys.exit(f"no depth-{DEPTH} loop in this kernel")
if TRACEBACK:
    head = max(per_loop, key=per_loop.get)
else:  # the sweep's step loops hold hundreds of vector instructions; an interior step is a boundary step less its guards
    steps = {k: v for k, v in per_loop.items() if v >= 100}
    head = min(steps, key=steps.get) if steps else max(per_loop, key=per_loop.get)
print(f"{'column' if TRACEBACK else 'interior step'} loop: {head}  ({per_loop[head]} vector instructions in its blocks; depth-{DEPTH} loops: {dict(per_loop)})")
inside = {n for n in order if blocks[n].loop == (head, DEPTH)}
HEAD = ".L" + head

RARE = ("global_atomic", "s_sleep", "flat_load", "flat_store")
is_dma = lambda o: o.startswith("global_load_lds")
is_steady_dma = lambda o: is_dma(o) and re.search(r"v\d+, s\[", o) is not None
is_wait = lambda o: o.startswith("s_waitcnt vmcnt(") and "lgkmcnt" not in o


def find_path(forbid, need, taken_first=False):
    """First path header -> header (depth first, in the order above) whose blocks hold no forbidden
    instruction and that holds at least one instruction of every kind in `need`."""
    dead = set()

    def ok(b):
        return not any(forbid(o) for o in b.ops)

    def walk(name, seen, have):
        b = blocks[name]
        have = have | frozenset(k for k, f in need.items() if any(f(o) for o in b.ops))
        key = (name, have)
        if key in dead:
            return None
        last = b.ops[-1].split()[0] if b.ops else ""
        succ = list(b.succ)
        if last == "s_cbranch_execnz" and len(succ) == 2:
            succ = [succ[0], succ[1]]   # some lane is active as a rule: into the guarded block first
        elif len(succ) == 2 and not (taken_first and last.startswith(("s_cbranch_scc", "s_cbranch_vcc"))):
            succ = [succ[1], succ[0]]   # fall-through first (for s_cbranch_execz: into the guarded block)
        for s in succ:
            if s == HEAD:
                if len(have) == len(need):
                    return [name]
                continue
            if s not in inside or s in seen or not ok(blocks[s]):
                continue
            r = walk(s, seen | {s}, have)
            if r:
                return [name] + r
        dead.add(key)
        return None

    return walk(HEAD, {HEAD}, frozenset()) if ok(blocks[HEAD]) else None


def report(title, path, sections):
    if not path:
        print(f"{title}: no such path")
        return
    ops = [o for n in path for o in blocks[n].ops]
    names = [o.split()[0] for o in ops]
    cls = lambda ns, p: sum(1 for o in ns if o.startswith(p))
    line = lambda ns: f"total {len(ns)}  VALU {cls(ns, 'v_')}  DS {cls(ns, 'ds_')}  SALU {cls(ns, 's_')}  VMEM {cls(ns, 'global_')}"
    print(f"{title}: {line(names)}")
    for o, c in collections.Counter(names).most_common(top):
        print(f"  {c:4d} {o}")
    mul = collections.Counter(n for n in names if n.startswith(("v_mad_u64", "v_mad_i64", "v_mul_")))
    print("  multiplies on the path:", dict(mul) if mul else "none")  # (a boundary path holds the step's own as well)
    if DUMP and not sections:
        print("\n".join("    | " + o for o in ops))
    if sections:
        rd = [i for i, n in enumerate(names) if n == "ds_read_b128"]
        wr = [i for i, n in enumerate(names) if n == "ds_write_b128"]
        dm = [i for i, o in enumerate(ops) if is_dma(o)]
        if rd and wr:
            print("  unpack section:", line(names[rd[0]:wr[-1] + 1]))
        if dm:
            first = (wr[-1] + 1) if wr and wr[-1] < dm[0] else next(i for i, o in enumerate(ops) if is_wait(o)) + 1
            sec = names[first:dm[-1] + 2]   # ... up to the last DMA's m0 restore
            print("  DMA section:   ", line(sec))
            mul = collections.Counter(n for n in sec if n.startswith(("v_mad_u64", "v_mad_i64", "v_mul_")))
            print("  multiplies in the DMA section:", dict(mul) if mul else "none")


rare = lambda o: o.startswith(RARE)
if TRACEBACK:
    need = {"load": lambda o: o.startswith("global_load"), "pick": lambda o: o.startswith("v_readlane")}
    wide = lambda o: o.startswith(("v_mad_i64", "v_mul_hi"))  # a division, a 64-bit product
    flush = lambda o: o.startswith(("global_store_byte", "s_barrier")) and "fast" in want
    path = find_path(lambda o: rare(o) or wide(o) or flush(o), need) or find_path(lambda o: rare(o) or flush(o), need)
    report("per-column common path", path, False)
    sys.exit(0)
# (the skip around the block-boundary work is a scalar branch either way round: both orders are tried, the shorter path
#  through a step's body -- its stores and its exchange -- is the step that does none of it)
step_body = {"store": lambda o: o.startswith("global_store"), "exchange": lambda o: o.startswith("ds_bpermute")}
hot = [p for p in (find_path(lambda o: rare(o) or is_dma(o) or is_wait(o), step_body, tf) for tf in (False, True)) if p]
report("per-step hot path", min(hot, key=lambda p: sum(len(blocks[n].ops) for n in p)) if hot else None, False)
loop_ops = [o for n in inside | {HEAD} for o in blocks[n].ops]
if any(is_steady_dma(o) for o in loop_ops):
    report("block-boundary path, steady block",
           find_path(lambda o: rare(o) or (is_dma(o) and not is_steady_dma(o)), {"dma": is_steady_dma, "wait": is_wait}), True)
report("block-boundary path, general block",
       find_path(lambda o: rare(o) or is_steady_dma(o), {"dma": is_dma, "wait": is_wait}), True)

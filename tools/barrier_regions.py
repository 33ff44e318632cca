"""Instructions by kind between the workgroup barriers of a cross-compiled listing:
    hipcc -O3 -std=c++17 -fno-strict-aliasing --offload-arch=gfx950 --cuda-device-only -S -o tile.s csrc/eaqhm_ls_tile.hip
    python tools/barrier_regions.py tile.s [--function tile_frame] [--x4 16]
One line per region (the text between two s_barrier of a function, in listing order): first line, instructions in all, and
how many are vector ALU, FP64 vector ALU, MFMA, scalar, LDS, global / flat memory, vector scratch, waits; `x4` is the number of
128-bit global or flat loads.  --x4 N shows only regions with at least N of them (tile_frame's gather has 4 per slot).
Last, the vector scratch instructions of each function over all its regions."""
import re
import sys


def kind(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu64" if "f64" in op else "valu"
    if op.startswith("s_waitcnt") or op == "s_nop":
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    return "other"


KINDS = ["valu", "valu64", "mfma", "salu", "lds", "vmem", "scratch", "wait", "other"]


def regions(path, want):
    """(function, first line, counts, 128-bit loads) of every barrier-to-barrier region of the functions whose name holds `want`."""
    fn, out, cur = None, [], None
    for no, line in enumerate(open(path), 1):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            fn = m.group(1) if want in m.group(1) else None
            cur = None
            if fn:
                cur = [fn, no, dict.fromkeys(KINDS, 0), 0]
                out.append(cur)
            continue
        if fn is None or not line.startswith("\t") or line.startswith("\t."):
            continue
        op = line.split()[0]
        if op.startswith(";"):
            continue
        if op == "s_barrier":
            cur = [fn, no, dict.fromkeys(KINDS, 0), 0]
            out.append(cur)
            continue
        cur[2][kind(op)] += 1
        if op in ("global_load_dwordx4", "flat_load_dwordx4"):
            cur[3] += 1
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    want = args[args.index("--function") + 1] if "--function" in args else ""
    x4 = int(args[args.index("--x4") + 1]) if "--x4" in args else 0
    last, total = None, {}
    for fn, no, c, n4 in regions(args[0], want):
        total[fn] = total.get(fn, 0) + c["scratch"]
        if n4 < x4:
            continue
        if fn != last:
            print(fn)
            last = fn
        print("  line %6d: %5d instructions | %s | x4 %d" % (no, sum(c.values()), " ".join("%s %d" % (k, c[k]) for k in KINDS if c[k]), n4))
    print("vector scratch instructions per function, all regions:")
    for fn, n in total.items():
        print("  %s %d" % (fn, n))

"""Device-code diff of the library against a git revision: does a refactor leave the machine code as it was?

    python tools/isa_diff.py [REV] [-D FLAG ...] [--rename OLD=NEW ...] [--keep DIR]

Builds the gfx950 device assembly of every source in csrc/Makefile's SRC, from the working tree and from REV (default
HEAD, extracted with git archive), with the Makefile's flags plus --offload-device-only -S and the -D flags given (to
both builds).  Each .s is normalised: comments, blank lines, .file / .loc / .ident directives and the __hip_cuid_*
symbol (it differs between two builds of the same source) are dropped, and the local labels (.LBB*, .Ltmp*,
.Lfunc_end*) are renumbered in order of appearance within each function.  A function's text runs from the directives
that open it (.text or, for a template's instantiation, its own .section ... comdat; .protected / .globl / .p2align
ahead of its .type) to those of the next one, or to the padding that closes the text section, so that a function added
next to it leaves it identical.  Reports every function (kernels and non-inlined device functions): identical, or
differs with its VGPR / AGPR / SGPR counts and scratch / LDS bytes before -> after.  --rename OLD=NEW (repeatable)
compares REV's function OLD with the working tree's NEW, for a kernel that changed its symbol (an extern "C" kernel that
became an instantiation of a kernel template: NEW is the mangled name): OLD is rewritten to NEW in REV's text of the
function, and the section directive that a comdat function has in place of .text is read as .text on both sides.  Exit
status 0 when every function and everything outside them compares equal.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = "eaqhm-analysis-and-synthesis-in-python_amd/csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fno-strict-aliasing", "--offload-arch=gfx950", "--offload-device-only", "-S"]

LABEL = re.compile(r"\.(LBB\d+_\d+|Ltmp\d+|Lfunc_end\d+)\b")
OPENERS = (".text", ".protected", ".globl", ".p2align", ".weak")
COMDAT = re.compile(r'^\s*\.section\s+\.text\.\S+,"axG",@progbits,\S+,comdat$')
FUNC = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
KD_FIELDS = {  # .amdhsa_* directive of the kernel descriptor -> column of the report
    "next_free_vgpr": "vgpr", "accum_offset": "agpr_off", "next_free_sgpr": "sgpr",
    "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}
SET_FIELDS = {"num_vgpr": "vgpr", "num_agpr": "agpr", "numbered_sgpr": "sgpr", "private_seg_size": "scratch"}


def sources(csrc):
    with open(os.path.join(csrc, "Makefile")) as fh:
        for line in fh:
            m = re.match(r"\s*SRC\s*:?=\s*(.*)", line)
            if m:
                return m.group(1).split()
    raise SystemExit("no SRC line in %s/Makefile" % csrc)


def build(csrc, out_dir, defines, jobs):
    os.makedirs(out_dir, exist_ok=True)
    srcs = sources(csrc)

    def one(src):
        out = os.path.join(out_dir, os.path.splitext(src)[0] + ".s")
        r = subprocess.run([HIPCC] + FLAGS + defines + ["-o", out, src], cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("%s failed in %s:\n%s" % (src, csrc, r.stderr))
        return src, out

    with ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, srcs))


def split(path):
    """Normalised text of a .s file: {function name: lines}, plus '<outside functions>'."""
    parts, cur, name = {}, [], "<outside functions>"
    with open(path) as fh:
        for raw in fh:
            line = raw.split(";", 1)[0].rstrip()
            s = line.strip()
            if not s or s.startswith(("//", ".file", ".loc", ".ident")) or "__hip_cuid_" in s:
                continue
            m = FUNC.match(line)
            if m or s.startswith((".amdgpu_metadata", ".p2alignl")):
                head = []   # what opens the next function (or the closing padding) is not the one before's
                while ((m or s.startswith(".p2alignl")) and cur
                       and (cur[-1].split()[0] in OPENERS or COMDAT.match(cur[-1]))):
                    head.insert(0, cur.pop())
                parts.setdefault(name, []).extend(cur)
                cur, name = head, (m.group(1) if m else "<outside functions>")
            cur.append(line)
    parts.setdefault(name, []).extend(cur)
    for k, lines in parts.items():
        ids = {}
        parts[k] = [LABEL.sub(lambda m: ".%s_%d" % (re.match(r"[A-Za-z_]+", m.group(1)).group(0),
                                                     ids.setdefault(m.group(1), len(ids))), l) for l in lines]
    return parts


def renamed(parts_old, parts_new, renames):
    """REV's function OLD under the working tree's name NEW; both without the comdat section directives."""
    for old, new in renames.items():
        if old not in parts_old or new in parts_old:
            continue
        word = re.compile(r"(?<![A-Za-z0-9_$])%s(?![A-Za-z0-9_$])" % re.escape(old))
        parts_old[new] = [word.sub(new, l) for l in parts_old.pop(old)]
        for parts in (parts_old, parts_new):
            if new in parts:
                parts[new] = ["\t.text" if COMDAT.match(l) else l for l in parts[new]]


def resources(lines):
    res = {}
    for l in lines:
        s = l.strip()
        m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", s)
        if m and m.group(1) in KD_FIELDS:
            res[KD_FIELDS[m.group(1)]] = m.group(2)
        m = re.match(r"\.set\s+\.?L?[^,]*\.(\w+),\s*(.*)", s)
        if m and m.group(1) in SET_FIELDS and SET_FIELDS[m.group(1)] not in res:
            res[SET_FIELDS[m.group(1)]] = m.group(2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor define for both builds")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="compare REV's function OLD with the working tree's function NEW")
    ap.add_argument("--keep", help="write the .s files under this directory and keep them")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    defines = ["-D" + d for d in a.defines]
    renames = dict(r.split("=", 1) for r in a.rename)
    was = {new: old for old, new in renames.items()}
    work = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    try:
        base_tree = os.path.join(work, "rev_tree")
        shutil.rmtree(base_tree, ignore_errors=True)
        os.makedirs(base_tree)
        arch = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC_REL, "include"], check=True,
                              capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base_tree], input=arch, check=True)
        with ThreadPoolExecutor(2) as ex:
            fb = ex.submit(build, os.path.join(base_tree, CSRC_REL), os.path.join(work, "rev"), defines, a.j)
            fw = ex.submit(build, os.path.join(ROOT, CSRC_REL), os.path.join(work, "tree"), defines, a.j)
            old, new = fb.result(), fw.result()
        same = True
        for src in sorted(set(old) | set(new)):
            if src not in old or src not in new:
                print("%s: only in %s" % (src, "the working tree" if src in new else a.rev))
                same = False
                continue
            po, pn = split(old[src]), split(new[src])
            renamed(po, pn, renames)
            print(src)
            for fn in sorted(set(po) | set(pn), key=lambda k: (k.startswith("<"), k)):
                lo, ln = po.get(fn), pn.get(fn)
                if lo == ln:
                    print("  identical  %s%s" % (fn, "  (was %s)" % was[fn] if fn in was else ""))
                    continue
                same = False
                if lo is None or ln is None:
                    print("  %s  %s" % ("added    " if lo is None else "removed  ", fn))
                    continue
                ro, rn = resources(lo), resources(ln)
                keys = [k for k in ("vgpr", "agpr", "agpr_off", "sgpr", "scratch", "lds") if k in ro or k in rn]
                nd = sum(1 for x, y in zip(lo, ln) if x != y) + abs(len(lo) - len(ln))
                print("  DIFFERS    %s%s  (%d of %d -> %d lines)"
                      % (fn, "  (was %s)" % was[fn] if fn in was else "", nd, len(lo), len(ln)))
                print("             " + "  ".join("%s %s -> %s" % (k, ro.get(k, "?"), rn.get(k, "?")) for k in keys))
        print("all identical" if same else "device code differs")
        return 0 if same else 1
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

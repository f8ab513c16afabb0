#!/usr/bin/env python3
"""Static ISA statistics of the ipm_kernel phases and sweeps (gfx950 assembly of scpp_hip.cpp).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip -ffp-contract=on --cuda-device-only -S -o /tmp/scpp.s scpp_amd/csrc/scpp_hip.cpp
  python tools/isa_round_trips.py /tmp/scpp.s [name-filter]

Per function: instructions, scratch dwords stored / loaded (callee-saved-register saves + spills), vector-memory operations, and
EXPOSED MEMORY ROUND TRIPS: an s_waitcnt vmcnt(N) counts when it covers an operation issued after the previous counted wait, i.e.
when the wavefront has to sit out a fresh memory latency (the hardware counter is in order, so vmcnt(N) waits for everything but
the N most recent operations).  All paths are counted (both sides of a branch), so the number is an upper bound per call.
The same rule on s_waitcnt lgkmcnt(N) gives the exposed LDS round trips: the issued operations are the LDS instructions (ds_*) and the
scalar loads (s_load_*, s_buffer_load_*), which share that counter.  With `--loop` the counts are also given for the MFMA loop of the
function alone (the innermost backward branch that encloses every v_mfma: the RKF78 step loop of the segment integration).
This is the measurement behind the round-2 restructuring of the phases: load groups closed by a scheduling
barrier, unconditional buffer accesses in the sweeps, chunk functions.  With `--skeleton name` it prints the order of load /
store / wait / MFMA / LDS groups of one function.
"""
import re
import sys

W = {"dword": 1, "dwordx2": 2, "dwordx3": 3, "dwordx4": 4, "b32": 1, "b64": 2, "b96": 3, "b128": 4}
VM_OP = r"(buffer|global|flat|scratch)_(load|store|atomic)"
LGKM_OP = r"^(ds_|s_load_|s_buffer_load_)"


def functions(path):
    funcs, cur = {}, None
    for l in open(path).read().split("\n"):
        m = re.match(r"^(_Z[\w]+):", l)
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is not None:
            funcs[cur].append(l)
    return funcs


def instructions(body, labels=False):
    pat = r"^\s+[vsbdg]\w*_" if not labels else r"^(\s+[vsbdg]\w*_|\.LBB)"
    return [l.split(";")[0].strip() for l in body if re.match(pat, l)]


def short(name):
    n = re.sub(r"_ZN4scpp3ipm(L?)\d+", "", name)
    return n[:44]


def round_trips(ins, op, counter):
    """(operations issued, exposed round trips) of one in-order counter: `op` matches what it counts, `counter` names it in s_waitcnt"""
    issued = done = last_rt = rts = 0
    for t in ins:
        if re.search(op, t):
            issued += 1
        m = re.match(r"s_waitcnt.*" + counter + r"\((\d+)\)", t)
        if m:
            cover = issued - int(m.group(1))
            if cover > done:
                if cover > last_rt:
                    rts += 1
                    last_rt = issued
                done = cover
    return issued, rts


def mfma_loop(body):
    """the instructions of the innermost loop (label .. backward branch to it) that holds every v_mfma of the function; None without one"""
    ins = instructions(body, labels=True)
    mf = [i for i, t in enumerate(ins) if "v_mfma" in t]
    if not mf:
        return None
    at = {t.rstrip(":"): i for i, t in enumerate(ins) if t.startswith(".LBB")}
    best = None
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", t)
        if m and at.get(m.group(1), i) < i and at[m.group(1)] <= mf[0] and i >= mf[-1]:
            if best is None or i - at[m.group(1)] < best[1] - best[0]:
                best = (at[m.group(1)], i)
    return None if best is None else [t for t in ins[best[0]:best[1] + 1] if not t.startswith(".LBB")]


def stats(path, flt):
    for name, body in functions(path).items():
        if ("3ipm" not in name and "--all" not in sys.argv) or (flt and flt not in name):
            continue
        ins = instructions(body)
        st = ld = 0
        for t in ins:
            m = re.search(r"scratch_(store|load)_(\w+)", t)
            if m:
                if m.group(1) == "store":
                    st += W.get(m.group(2), 1)
                else:
                    ld += W.get(m.group(2), 1)
        issued, rts = round_trips(ins, VM_OP, "vmcnt")
        lgkm, lrts = round_trips(ins, LGKM_OP, "lgkmcnt")
        print(f"{short(name):46s} ins {len(ins):5d}  scratch st/ld dwords {st:4d}/{ld:4d}  vm ops {issued:4d}  exposed round trips {rts:4d}"
              f"  mfma {sum('v_mfma' in t for t in ins):3d}  lds {sum(t.startswith('ds_') for t in ins):4d}  lgkm ops {lgkm:4d}  exposed lgkm round trips {lrts:4d}")
        if "--loop" in sys.argv:
            lp = mfma_loop(body)
            if lp:
                v = round_trips(lp, VM_OP, "vmcnt")
                k = round_trips(lp, LGKM_OP, "lgkmcnt")
                print(f"{'    mfma loop':46s} ins {len(lp):5d}  vm ops {v[0]:4d}  exposed round trips {v[1]:4d}  mfma {sum('v_mfma' in t for t in lp):3d}"
                      f"  lgkm ops {k[0]:4d}  exposed lgkm round trips {k[1]:4d}  s_and_saveexec {sum('s_and_saveexec' in t for t in lp):3d}")


def skeleton(path, flt):
    for name, body in functions(path).items():
        if flt not in name:
            continue
        print(name)
        prev, n = None, 0
        for i, t in enumerate(instructions(body, labels=True)):
            kind = None
            if t.startswith("s_waitcnt") and ("vmcnt" in t or "lgkmcnt" in t):
                kind = "WAIT " + t
            elif re.search(r"(global|buffer|scratch)_store", t):
                kind = "store"
            elif re.search(r"(global|buffer|scratch|flat)_load", t):
                kind = "load"
            elif re.match(r"ds_(read|load)", t):
                kind = "ds_read"
            elif t.startswith("ds_"):
                kind = "ds_write" if re.match(r"ds_(write|store)", t) else "ds_other"
            elif "v_mfma" in t:
                kind = "mfma"
            elif t.startswith(".LBB"):
                kind = "LABEL " + t
            elif "s_cbranch" in t or "s_branch" in t or "s_swappc" in t:
                kind = "BR " + t
            elif "s_and_saveexec" in t:
                kind = "saveexec"
            if kind:
                if kind == prev:
                    n += 1
                else:
                    if prev and n > 1:
                        print("        x", n)
                    print(f"{i:6d} {kind}")
                    n = 1
                prev = kind
        return


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a not in ("--all", "--loop")]
    if len(args) > 2 and args[1] == "--skeleton":
        skeleton(args[0], args[2])
    else:
        stats(args[0], args[1] if len(args) > 1 else "RocketQuat")

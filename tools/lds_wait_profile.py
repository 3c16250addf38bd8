"""Where does the step kernel wait for LDS right behind the read it waits for?  Reads the device assembly tools/static_phase_profile.py
reads (made with -gline-tables-only; the hipcc line and the awk cut of one kernel stand there) and reports, per phase, the number of
`s_waitcnt` that name lgkmcnt and how many of them sit within NEAR (8) vector instructions of the last LDS read issued (`ds_read*`,
`ds_bpermute*`): a wait that close behind its read is a round trip the wave pays in full unless another wave fills it.

  python tools/lds_wait_profile.py /tmp/k.s [--json] [--src DIR]      (DIR: the csrc/ the assembly was made from, another revision's for A/B)

A phase is what tools/stamps.py times: the code of mocca_device.h up to the next STAMP(n) of the function it is inlined from (named as in
stamps.py's SEQ), or that function's name where no STAMP follows.  Static, as static_phase_profile.py is: loops that are not unrolled
count once.  Only the opcodes of waits, LDS reads and vector instructions are looked at.  Run from the repo root."""
import bisect
import json
import re
import sys

NEAR = 8
SKIP = {"mocca_step_kernel", "substep", "env_step_impl"}
# STAMP id -> the phase it ENDS (tools/stamps.py SEQ)
STAMP_NAMES = {29: "stage joints", 0: "kinematics walk", 15: "geom points", 13: "collide: terrain", 14: "collide: self pairs",
               1: "collide: epilogue", 10: "aba: inward levels", 11: "aba: base 6x6", 12: "aba: outward walk", 2: "aba: epilogue",
               16: "rows: limit compaction", 17: "rows: build row", 5: "rows: ancestor masks", 18: "sweeps: anymask reduction",
               19: "sweeps: inward", 6: "sweeps: base + outward", 7: "Delassus build", 20: "pgs: warm start", 8: "pgs: iterations",
               9: "apply", 3: "solve: epilogue", 4: "integrate"}


def source_tables(text):
    """source text of a header -> (function starts [(line, name)], stamps [(line, id)])"""
    starts, stamps = [], []
    for i, ln in enumerate(text.splitlines(), 1):
        m = re.match(r"^DI\s+[\w:<>\*&\s]+?\b(\w+)\s*\(", ln) or re.match(r"^__global__.*\b(\w+)\s*\(", ln)
        if m:
            starts.append((i, m.group(1)))
        m = re.match(r"^\s*STAMP\((\d+)\);", ln)
        if m:
            stamps.append((i, int(m.group(1))))
    return starts, stamps


def make_phase_of(tables):
    """tables {file name: source_tables(...)} -> phase_of(frames), frames = [(file, line), ...] innermost first as a .loc comment lists them"""
    def func_at(f, line):
        if f not in tables:
            return None, 0, 1 << 30
        starts = tables[f][0]
        i = bisect.bisect_right([s[0] for s in starts], line) - 1
        if i < 0:
            return None, 0, 1 << 30
        return starts[i][1], starts[i][0], starts[i + 1][0] if i + 1 < len(starts) else 1 << 30

    def phase_of(frames):
        for f, line in frames[::-1]:   # outermost first
            f = f.split("/")[-1]
            name, lo, hi = func_at(f, line)
            if name is None or name in SKIP:
                continue
            for sl, sid in tables[f][1]:
                if lo <= sl < hi and sl > line and sid in STAMP_NAMES:
                    return STAMP_NAMES[sid]
            return name
        return "kernel body"
    return phase_of


def profile(asm_lines, phase_of):
    """-> {phase: {"waits": n, "near": n, "lds_reads": n}}; a wait is near if at most NEAR vector instructions were issued since the last LDS read"""
    out, cur, since = {}, "?", None
    for ln in asm_lines:
        if re.match(r"\s*\.loc\s", ln):
            fr = re.findall(r"([^\s:\[\]@;]+):(\d+):\d+", ln.split(";", 1)[1]) if ";" in ln else []
            fr = [(f, int(n)) for f, n in fr if int(n)]
            if fr:
                cur = phase_of(fr)
            continue
        t = ln.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        rec = out.setdefault(cur, {"waits": 0, "near": 0, "lds_reads": 0})
        if op.startswith("ds_read") or op.startswith("ds_bpermute"):
            rec["lds_reads"] += 1
            since = 0
        elif op == "s_waitcnt" and "lgkmcnt" in t:
            rec["waits"] += 1
            if since is not None and since <= NEAR:
                rec["near"] += 1
        elif op.startswith("v_") and since is not None:
            since += 1
    return out


if __name__ == "__main__":
    src = sys.argv[sys.argv.index("--src") + 1] if "--src" in sys.argv else "mocca_envs_amd/csrc"   # the sources the assembly was made from
    srcs = {"mocca_device.h": src + "/mocca_device.h", "mocca_kernels.h": src + "/mocca_kernels.h"}
    res = profile(open(sys.argv[1]), make_phase_of({k: source_tables(open(p).read()) for k, p in srcs.items()}))
    if "--json" in sys.argv:
        print(json.dumps(res, indent=1))
    else:
        print("%-32s %6s %6s %9s" % ("phase", "waits", "near", "LDS reads"))
        for k, v in sorted(res.items(), key=lambda kv: -kv[1]["waits"]):
            if v["waits"]:
                print("%-32s %6d %6d %9d" % (k, v["waits"], v["near"], v["lds_reads"]))
        print("%-32s %6d %6d %9d" % ("total", *(sum(v[f] for v in res.values()) for f in ("waits", "near", "lds_reads"))))

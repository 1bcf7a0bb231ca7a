#!/usr/bin/env python3
"""Register / scratch / LDS / occupancy table of the env step kernels from hipcc's resource-usage remarks.

    hipcc <the flags of _capi.HIPCC_FLAGS> -Rpass-analysis=kernel-resource-usage -c csrc/usv_env.hip 2> remarks.txt
    python tools/env_resource_usage.py parent=parent_remarks.txt branch=remarks.txt

Prints one table per LABEL=FILE argument (every k_env_step* instantiation), then the rows that differ between the
first and the second file.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("SGPRs Spill", "SGPR spill"), ("VGPRs Spill", "VGPR spill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occ"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"\(StepCfg.*$", "", ln.replace("(anonymous namespace)::", "").replace("void ", ""))
            for ln in out.splitlines()]


def parse(path):
    rows, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: (?:\S+:\d+:\d+: +)?(.*?) \[-Rpass-analysis", ln)   # location before or after "remark:"
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(": ")
        if key == "Function Name":
            cur = rows.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    names = [k for k in rows if "k_env_step" in k]
    return dict(zip(demangle(names), (rows[k] for k in names)))


def table(label, rows):
    w = max(len(k) for k in rows)
    print(f"== {label}")
    print(f"{'kernel':<{w}} " + " ".join(f"{h:>10}" for _, h in FIELDS))
    for k in sorted(rows):
        print(f"{k:<{w}} " + " ".join(f"{rows[k].get(f, '?'):>10}" for f, _ in FIELDS))
    print()


def main():
    tabs = [(a.partition("=")[0], parse(a.partition("=")[2])) for a in sys.argv[1:]]
    for label, rows in tabs:
        table(label, rows)
    if len(tabs) >= 2:
        (la, a), (lb, b) = tabs[:2]
        print(f"== rows that differ ({la} -> {lb})")
        n = 0
        for k in sorted(set(a) | set(b)):
            d = [f"{h} {a.get(k, {}).get(f, '-')} -> {b.get(k, {}).get(f, '-')}" for f, h in FIELDS
                 if a.get(k, {}).get(f) != b.get(k, {}).get(f)]
            if d:
                n += 1
                print(f"{k}: " + ", ".join(d))
        print(f"{n} of {len(set(a) | set(b))} kernels differ")


if __name__ == "__main__":
    main()

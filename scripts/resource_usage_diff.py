#!/usr/bin/env python3
"""Compares two builds' -Rpass-analysis=kernel-resource-usage remarks, kernel by kernel under the demangled name.

    hipcc <flags> -Rpass-analysis=kernel-resource-usage -c csrc/X.hip -o /dev/null 2> X.remarks      (both trees)
    resource_usage_diff.py --what TEXT --out profiles/NAME.json X.hip=parent/X.remarks:new/X.remarks [...]

A new kernel whose name is that of an existing one with `_many` before `_kernel` is listed beside that twin's instance of
the same leading template arguments (the one-record kernel whose body it runs)."""
from __future__ import annotations

import argparse
import json
import re
import subprocess

FIELDS = [("TotalSGPRs", "sgprs"), ("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("ScratchSize [bytes/lane]", "scratch_bytes_per_lane"),
          ("Occupancy [waves/SIMD]", "occupancy_waves_per_simd"), ("SGPRs Spill", "sgpr_spills"), ("VGPRs Spill", "vgpr_spills"),
          ("LDS Size [bytes/block]", "lds_bytes")]


def parse(path: str) -> dict:
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+) \[-Rpass", line)
        if m and cur is not None:
            for label, key in FIELDS:
                if m.group(1).strip() == label:
                    cur[key] = int(m.group(2))
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(.*$", "", d): out[n] for n, d in zip(names, dem)}


def twin_of(name: str, old: dict):
    m = re.match(r"(.*)_many_kernel<(.*)>$", name)
    if not m:
        return None
    args = [a.strip() for a in m.group(2).split(",")]
    best = None
    for cand in old:
        c = re.match(re.escape(m.group(1)) + r"_kernel<(.*)>$", cand)
        if not c:
            continue
        cargs = [a.strip() for a in c.group(1).split(",")]
        # the twin's arguments with its defaulted ones (PROBE = 0) dropped are the many kernel's
        if [a for a in cargs if a != "0"] == args or cargs == args:
            best = cand
    return best


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--note", action="append", default=[])
    ap.add_argument("pairs", nargs="+", help="FILE=parent.remarks:new.remarks")
    a = ap.parse_args()
    doc = {"what": a.what, "files": {}}
    for pair in a.pairs:
        label, paths = pair.split("=", 1)
        old, new = (parse(p) for p in paths.split(":"))
        changed = {k: {"parent": old[k], "this_change": new[k]} for k in old if k in new and old[k] != new[k]}
        added = {}
        for k in new:
            if k in old:
                continue
            t = twin_of(k, new)
            added[k] = dict(new[k], **({"one_record_twin": t, "twin": new[t]} if t else {}))
        doc["files"][label] = {
            "kernels_in_parent": len(old), "kernels_in_this_change": len(new),
            "kernels_with_identical_resource_usage": sum(1 for k in old if k in new and old[k] == new[k]),
            "kernels_removed": sorted(k for k in old if k not in new),
            "kernels_changed": changed,
            "kernels_changed_in_more_than_sgprs": sorted(k for k, v in changed.items()
                                                         if any(v["parent"][f] != v["this_change"][f] for _, f in FIELDS if f != "sgprs")),
            "largest_sgpr_difference": max([abs(v["parent"]["sgprs"] - v["this_change"]["sgprs"]) for v in changed.values()] or [0]),
            "kernels_added": added,
            "many_kernels_below_their_twin": sorted(k for k, v in added.items() if "twin" in v and (
                v["occupancy_waves_per_simd"] < v["twin"]["occupancy_waves_per_simd"] or v["scratch_bytes_per_lane"] or v["vgpr_spills"] or v["sgpr_spills"])),
        }
    if a.note:
        doc["notes"] = a.note
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for label, d in doc["files"].items():
        print(label, {k: (len(v) if isinstance(v, (dict, list)) else v) for k, v in d.items()})


if __name__ == "__main__":
    main()

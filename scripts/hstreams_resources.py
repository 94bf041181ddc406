#!/usr/bin/env python3
"""Development aid: the rows of profiles/hstreams_kernel_resources.txt.  Compiles the device translation units of a source tree
(kernels.hip and, where the tree has it, kernels_hstreams.hip) for gfx950 with hipcc's resource-usage remarks and prints one
row per kernel named below, in the format of scripts/kernel_resources.sh.  No GPU is needed.

    scripts/hstreams_resources.py [TREE]      (TREE: a checkout of this repository; default: this one)
"""
import os
import re
import subprocess
import sys
import tempfile

KERNELS = ["_Z20k_encode_hc_fstreams12FStreamsArgsi", "_Z11k_encode_hc10EncodeArgsi", "_Z16k_encode_hc_dict10HcDictArgsi",
           "_Z17k_encode_fstreamsILb0EEv12FStreamsArgs", "_Z17k_encode_fstreamsILb1EEv12FStreamsArgs"]
FIELDS = [("vgpr", "VGPRs", 3), ("sgpr", "TotalSGPRs", 3), ("vspill", "VGPRs Spill", 2), ("sspill", "SGPRs Spill", 3),
          ("lds", "LDS Size [bytes/block]", 6), ("scratch", "ScratchSize [bytes/lane]", 4)]


def remarks(tree, unit):
    src = os.path.join(tree, "streamly-lz4_amd", "csrc", unit)
    if not os.path.exists(src):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(tmp, "unit.o"), "-x", "hip", src],
                           capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-4000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main():
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {}
    for unit in ("kernels.hip", "kernels_hstreams.hip"):
        seen.update(remarks(tree, unit))
    for name in KERNELS:
        if name in seen:
            print("%-60s %s" % (name, " ".join("%s %*s" % (tag, w, seen[name][key]) for tag, key, w in FIELDS)))


if __name__ == "__main__":
    main()

"""Development aid: a batch whose records belong to many dictionaries, through the dictionary-set calls and through
the single-dictionary calls they stand beside, all timed in one session.  16384 text records of 4 KiB, 64 members of 64 KiB of the
same generator's text, 256 records a member:
  (a) one mi355lz4_compress_fastdict_multi_device call, the members' records shuffled through the batch;
  (b) one such call, the records sorted by member;
  (c) 64 mi355lz4_compress_fastdict_device calls of 256 records, back to back, timed as one window;
  (d) one mi355lz4_compress_fastdict_device call over all records against one member: the floor, (b) - (d) is the grouping pass;
  (e) a skewed batch -- 32 members with 1024 records of 1 KiB each, 32 with 64 records of 16 KiB each, the same 64 MiB, sorted by
      member -- through the multi call and through one single-dictionary call on the same lengths: what equal block counts per
      wave cost when the lengths go with the dictionary.
The decode side the same way for (a), (c) and (d): mi355lz4_decompress_dict_multi_device against mi355lz4_decompress_dict_device.
Every call is device-resident and event-timed on the engine's stream: one warm-up call per form, then `REPS` rounds in which the
forms alternate; a record holds the five times and their median.  "separated": (a)'s five values all lie below (c)'s five.
Everything the multi calls wrote is decoded and compared with its source.
    timeout -k 10 600 python3 scripts/dictset_rate.py [OUT.json [COMMIT]]
OUT.json defaults to profiles/dictset_rate.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
DICT, MEMBERS, BL, N, REPS = 65536, 64, 4096, 16384, 5
PER = N // MEMBERS


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(dev)


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(dev)


def alternate(forms):
    """forms: {name: fn}.  One warm-up call each, then REPS rounds over all forms: {name: {"ms": [...], "median_ms": m}}"""
    for fn in forms.values():
        fn()
    eng.synchronize()
    ts = {k: [] for k in forms}
    for _ in range(REPS):
        for name, fn in forms.items():
            a, b = S.Event(), S.Event()
            eng.record(a)
            fn()
            eng.record(b)
            eng.synchronize()
            ts[name].append(S.Engine.elapsed_ms(a, b))
    return {k: {"ms": v, "median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}


def verdict(rec, a, c):
    rec["a_below_c"] = rec[a]["median_ms"] < rec[c]["median_ms"]
    rec["separated"] = rec[a]["max_ms"] < rec[c]["min_ms"]


# ---- the members and the records -------------------------------------------------------------------------------------------------
dicts = torch.empty(MEMBERS * DICT, dtype=torch.uint8, device=dev)
eng.generate("text", dicts, BL, MEMBERS * DICT // BL, first_block=N + 7)
members = []
for k in range(MEMBERS):
    hd = S.HcDict(eng)
    hd.load(dicts[k * DICT:(k + 1) * DICT], DICT)
    members.append(hd)
ds = S.DictSet(eng, members)
src = torch.empty(N * BL, dtype=torch.uint8, device=dev)
eng.generate("text", src, BL, N)
eng.synchronize()

sorted_idx = np.repeat(np.arange(MEMBERS), PER)
shuffled_idx = np.random.RandomState(20261020).permutation(sorted_idx)
idx_sorted, idx_shuffled, idx_one = i32(sorted_idx), i32(shuffled_idx), i32(np.zeros(N))
stride = S.slot_stride(BL, 8)
slots = {k: torch.empty(N * stride, dtype=torch.uint8, device=dev) for k in "abcd"}
flen = {k: torch.zeros(N, dtype=torch.int32, device=dev) for k in "abcd"}


def c_compress():
    for k in range(MEMBERS):
        lo = k * PER
        eng.compress_fastdict_device(members[k], src[lo * BL:], PER, BL, slots["c"][lo * stride:], stride, flen["c"][lo:])


record = {"shape": {"kind": "text", "block": BL, "blocks": N, "members": MEMBERS, "dictionary": DICT, "reps": REPS}}
comp = alternate({
    "a_multi_shuffled": lambda: eng.compress_fastdict_multi_device(ds, idx_shuffled, src, N, BL, slots["a"], stride, flen["a"]),
    "b_multi_sorted": lambda: eng.compress_fastdict_multi_device(ds, idx_sorted, src, N, BL, slots["b"], stride, flen["b"]),
    "c_64_single_calls": c_compress,
    "d_one_single_call": lambda: eng.compress_fastdict_device(members[0], src, N, BL, slots["d"], stride, flen["d"]),
})
eng.compress_fastdict_multi_device(ds, idx_shuffled, src, N, BL, slots["a"], stride, flen["a"])
comp["a_stagings_grid"] = list(ds.last())
comp["grouping_pass_ms"] = comp["b_multi_sorted"]["median_ms"] - comp["d_one_single_call"]["median_ms"]
comp["b_over_d"] = comp["b_multi_sorted"]["median_ms"] / comp["d_one_single_call"]["median_ms"]
comp["same_bytes_b_c"] = bool(torch.equal(flen["b"], flen["c"])) and bool(torch.equal(slots["b"].view(N, stride)[:, :64], slots["c"].view(N, stride)[:, :64]))
for k in "abcd":
    comp["ratio_" + k] = N * BL / (int(flen[k].sum().item()) - 8 * N)
verdict(comp, "a_multi_shuffled", "c_64_single_calls")
record["compress"] = comp

# ---- decode ----------------------------------------------------------------------------------------------------------------------
out = {k: torch.empty(N * BL, dtype=torch.uint8, device=dev) for k in "acd"}
res = {k: torch.zeros(N, dtype=torch.int32, device=dev) for k in "acd"}
boff = torch.arange(N, dtype=torch.int64, device=dev) * stride
ooff = torch.arange(N + 1, dtype=torch.int64, device=dev) * BL


def c_decode():
    for k in range(MEMBERS):
        lo = k * PER
        eng.decompress_dict_device(slots["c"][lo * stride:], PER * stride, boff, PER, dicts[k * DICT:], DICT, out["c"][lo * BL:], ooff,
                                   res["c"][lo:])


dec = alternate({
    "a_multi_shuffled": lambda: eng.decompress_dict_multi_device(slots["a"], N * stride, boff, N, ds, idx_shuffled, out["a"], ooff, res["a"]),
    "c_64_single_calls": c_decode,
    "d_one_single_call": lambda: eng.decompress_dict_device(slots["d"], N * stride, boff, N, dicts, DICT, out["d"], ooff, res["d"]),
})
dec["decodes"] = all(bool(torch.equal(out[k], src)) and res[k].tolist() == [BL] * N for k in "acd")
verdict(dec, "a_multi_shuffled", "c_64_single_calls")
record["decode"] = dec

# ---- (e) lengths that go with the dictionary -------------------------------------------------------------------------------------
lens = np.concatenate([np.full(32 * 1024, 1024), np.full(32 * 64, 16384)]).astype(np.int64)
member_of = np.concatenate([np.repeat(np.arange(32), 1024), np.repeat(np.arange(32, 64), 64)])
ne = lens.size
offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
estride = S.slot_stride(16384, 8)
eslots = torch.empty(ne * estride, dtype=torch.uint8, device=dev)
eflen = torch.zeros(ne, dtype=torch.int32, device=dev)
e_off, e_len, e_idx = i64(offs), i32(lens), i32(member_of)
skew = alternate({
    "multi_sorted": lambda: eng.compress_fastdict_multi_device(ds, e_idx, src, ne, 16384, eslots, estride, eflen, src_off=e_off, src_len=e_len,
                                                               block_stride=0),
    "one_single_call": lambda: eng.compress_fastdict_device(members[0], src, ne, 16384, eslots, estride, eflen, src_off=e_off, src_len=e_len,
                                                            block_stride=0),
})
skew["blocks"] = int(ne)
skew["multi_over_single"] = skew["multi_sorted"]["median_ms"] / skew["one_single_call"]["median_ms"]
record["e_skewed"] = skew

record["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dictset_rate.json")
if len(sys.argv) > 2:
    record["commit"] = sys.argv[2]
print(json.dumps(record), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(record, f, indent=1)
ds.close()
for hd in members:
    hd.close()
eng.close()

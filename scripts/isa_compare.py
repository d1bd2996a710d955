"""Compare llvm-objdump -d outputs kernel by kernel: instruction text only (addresses, encodings, label numbers stripped)."""
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        ins = line.split("//")[0].strip()
        if not ins:
            continue
        ins = re.sub(r"<[^>]*>", "<L>", ins)  # branch targets
        out[cur].append(ins)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
# the MIX = false instantiations under the names they had: without the extra template flag and trailing CeMix<false>
b = {re.sub(r"NS_5CeMixIXT\d_EEE$", "", re.sub(r"(Lb[01]E)Lb0E(EEv)", r"\1\2", k)): v for k, v in b.items()}
same = diff = 0
for k, v in a.items():
    if k not in b:
        print("MISSING in new:", k)
        diff += 1
    elif v != b[k]:
        n = next((i for i, (x, y) in enumerate(zip(v, b[k])) if x != y), min(len(v), len(b[k])))
        print(f"DIFF {k}: {len(v)} vs {len(b[k])} instructions, first at {n}: {v[n] if n < len(v) else None} | {b[k][n] if n < len(b[k]) else None}")
        diff += 1
    else:
        same += 1
print(f"{same} identical, {diff} different; new-only kernels: {len(set(b) - set(a))}; instructions compared: {sum(len(v) for v in a.values())}")

"""Instruction counts per wave of every resblock_x3_kernel instantiation, from the compiler's assembly of csrc/resnet.hip.

    hipcc <build.py CFLAGS> --cuda-device-only -S -o resnet.s cough_detector_amd/csrc/resnet.hip
    python tools/rbx_isa_count.py resnet.s [other.s ...]

Per instantiation: VGPRs and scratch from the kernel's metadata, then the instructions of the straight-line code by phase
-- before the first MFMA (staging), conv1 + projection (first MFMA to the barrier in front of the h write), the h write,
conv2 (to the last MFMA) and after it.  Columns: MFMA, other vector (v_*), LDS (ds_*), vector memory (global_*), s_nop,
v_cndmask, additions of the LDS base (`v_add_u32 v, 0, v`) and 64-bit vector additions (v_addc_co_u32).  The kernels are
fully unrolled, so a count is what one wave issues -- but the 32x32x16 body holds two bodies, of which a wave runs one,
and a two-clip instantiation holds its staging twice (the last workgroup's instance lands behind the last MFMA).
"""
import re
import sys

NAME = re.compile(r"^_ZN5cough12_GLOBAL__N_118resblock_x3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEvNS0_7RbxArgsE:")
COLS = ("mfma", "valu", "lds", "vmem", "s_nop", "cndmask", "add0", "addc")


def classify(op, args):
    if op.startswith("v_mfma"):
        return ["mfma"]
    out = []
    if op.startswith("v_"):
        out.append("valu")
        if op.startswith("v_cndmask"):
            out.append("cndmask")
        if op.startswith("v_addc_co_u32"):
            out.append("addc")
        if op.startswith("v_add_u32") and re.match(r"v\d+, 0, v\d+$", args):
            out.append("add0")
    elif op.startswith("ds_"):
        out.append("lds")
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        out.append("vmem")
    elif op == "s_nop":
        out.append("s_nop")
    return out


def kernels(path):
    cur, body, meta = None, [], {}
    for ln in open(path):
        m = NAME.match(ln)
        if m:
            cur, body = tuple(int(x) for x in m.groups()), []
            continue
        if cur is None:
            continue
        s = ln.strip()
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            if s.startswith(".Lfunc_end") and cur not in meta:
                meta[cur] = {"body": body}
            continue
        m = re.match(r"; (NumVgprs|ScratchSize): (\d+)", s)
        if m and cur in meta:
            meta[cur].setdefault(m[1], int(m[2]))   # the first after the body: later functions of the file follow
            continue
        if s and not s.startswith((";", ".")) and not s.endswith(":") and cur not in meta:
            parts = s.split(None, 1)
            body.append((parts[0], parts[1].split(";")[0].strip() if len(parts) > 1 else ""))
    return meta


def phases(body):
    """Indices splitting the body: first MFMA, the barrier that opens the h write, the MFMA that follows it, last MFMA."""
    mf = [i for i, (op, _) in enumerate(body) if op.startswith("v_mfma")]
    first, last = mf[0], mf[-1]
    # the h write lies between the two s_barrier that have MFMAs on both sides and the largest MFMA-free gap
    gaps = [(b - a, a, b) for a, b in zip(mf, mf[1:]) if any(body[k][0] == "s_barrier" for k in range(a, b))]
    _, a, b = max(gaps)
    return first, a + 1, b, last + 1


def main():
    for path in sys.argv[1:]:
        print(path)
        print("  %-22s %5s %7s | %-12s" % ("instantiation", "VGPRs", "scratch", "phase") + "".join("%8s" % c for c in COLS))
        for key, k in sorted(kernels(path).items()):
            body = k["body"]
            f, h0, h1, l = phases(body)
            spans = (("staging", 0, f), ("conv1+proj", f, h0), ("h write", h0, h1), ("conv2", h1, l), ("epilogue", l, len(body)),
                     ("k-loops", None, None), ("kernel", 0, len(body)))
            name = "<%d,%d,%d,%d,%d>" % key
            for pname, a, b in spans:
                rows = body[f:h0] + body[h1:l] if a is None else body[a:b]
                cnt = dict.fromkeys(COLS, 0)
                for op, args in rows:
                    for c in classify(op, args):
                        cnt[c] += 1
                print("  %-22s %5s %7s | %-12s" % (name, k.get("NumVgprs", "?"), k.get("ScratchSize", "?"), pname) +
                      "".join("%8d" % cnt[c] for c in COLS))
                name = ""


if __name__ == "__main__":
    main()

"""Device assembly of wgrad.hip, dense_chain.hip, conv_thin.hip, resample.hip, the view kernels' or the degradation kernels' files, one tree against another, per kernel (the method of
profiles/conv_igemm_refactor_isa.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I. --offload-device-only -S -o parent.s <parent>/wgrad.hip      (same for the branch)
    python tools/wgrad_isa_compare.py parent.s branch.s > profiles/wgrad_refactor_isa.txt
    python tools/wgrad_isa_compare.py --kernel dense_chain parent.s branch.s > profiles/dense_chain_refactor_isa.txt
    python tools/wgrad_isa_compare.py --kernel thin parent.s branch.s > profiles/conv_thin_refactor_isa.txt
    python tools/wgrad_isa_compare.py --kernel resample parent.s branch.s > profiles/resample_refactor_isa.txt
    cat <parent>/{elementwise,loss,layout,norm,resample}.s > parent.s  (same for the branch)
    python tools/wgrad_isa_compare.py --kernel views parent.s branch.s > profiles/view_kernels_refactor_isa.txt
    cat <parent>/{degrade,blur_f64,jpeg}.s > parent.s ; cat <branch>/{degrade,filter2d,jpeg}.s > branch.s
    python tools/wgrad_isa_compare.py --kernel degrade parent.s branch.s > profiles/degrade_refactor_isa.txt

wgrad kernels are matched by template arguments <T, KS, STRIDE, XP, YP, DMA>; a seventh argument (the parent's VAR) is dropped;
dense-chain kernels by <T, RPW>; the thin-side kernels by <T, MASK, NT> (thin_in) and <T> (thin_out, thin_wgrad), the slab reduction by
its symbol.  Per kernel: the .amdhsa_kernel block, and the counts of MFMA, LDS, global / flat / scratch memory,
buffer, s_waitcnt and s_barrier instructions, which must be equal; --kernel dense_chain and --kernel thin also count v_readlane / v_writelane (SGPR
spills to lanes), which must not rise.  --kernel resample matches resample_vec_kernel<T, OP> / relu_copy_vec_kernel<T> and the five
scalar kernels of the old file to resample_kernel<T, N, OP>, the row-grid kernels by <T> and <T, NT>; the scalar forms (N = 1) are
reported as what they became, not held to the counts.  --kernel views (elementwise.hip, loss.hip, layout.hip, norm.hip, and resample.hip,
whose labels are those of --kernel resample) matches the scalar / vector pairs of the old files (x_kernel<T> / x_vec_kernel<T>) to
x_kernel<T, N>, the three per-pixel RGB kernels to rgb_to_nhwc_kernel<T, CLAMP, WIDE>, the four one-block sums to finish_kernel<E>, and
every other kernel by name and element type, whatever its arguments became; scalar forms are reported, axpby_kernel<f32, scalar> aside
(the trainers run it); an s_waitcnt count that moved is listed, and fails only if the waits on vector memory (vmcnt) moved.
--kernel degrade (degrade.hip, filter2d.hip / blur_f64.hip, jpeg.hip) matches kernels by name and template arguments, which the refactor kept.
Held per kernel: LDS bytes, no scratch, the counts of global loads, global stores, LDS reads, LDS writes and barriers, the waves-per-SIMD step
of the VGPR count; scalar loads and s_waitcnt are counted and listed where they moved, not held.
A working tool, not a test."""
import collections
import re
import sys

NAME = re.compile(r"wgrad_kernelI(t|DF16_|f)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E(?:Li(\d+)E)?E")
DC_NAME = re.compile(r"dense_chain_kernelI(t|DF16_)Li(\d+)EE")
THIN_NAME = re.compile(r"(thin_in|thin_out|thin_wgrad)_kernelI(t|DF16_)(?:Lb(\d)ELb(\d)E)?E")
RS_T = r"I(t|DF16_|f)"
RS_NAMES = [   # (pattern, label format): groups are (T, ...)
    (re.compile(r"resample_vec_kernel" + RS_T + r"Li(\d)EE"), lambda g: "resample_kernel<%s, vec, OP=%s>" % (TYPES[g[0]], g[1])),
    (re.compile(r"relu_copy_vec_kernel" + RS_T + "E"), lambda g: "resample_kernel<%s, vec, OP=4>" % TYPES[g[0]]),
    (re.compile(r"\d\d(up2_nearest_bwd|up2_bilinear_fwd|up2_bilinear_bwd|maxpool2|relu_copy)_kernel" + RS_T + "E"),
     lambda g: "resample_kernel<%s, scalar, OP=%d>" % (TYPES[g[1]], ["up2_nearest_bwd", "up2_bilinear_fwd", "up2_bilinear_bwd", "maxpool2", "relu_copy"].index(g[0]))),
    (re.compile(r"resample_kernel" + RS_T + r"Li(\d)ELi(\d)EE"), lambda g: "resample_kernel<%s, %s, OP=%s>" % (TYPES[g[0]], "scalar" if g[1] == "1" else "vec", g[2])),
    (re.compile(r"bilinear_up2_(?:block|rows)_kernel" + RS_T + "E"), lambda g: "bilinear_up2_rows_kernel<%s>" % TYPES[g[0]]),
    (re.compile(r"bilinear_up2_bwd_rows_kernel" + RS_T + r"(?:Li4E)?Lb(\d)EE"), lambda g: "bilinear_up2_bwd_rows_kernel<%s, NT=%s>" % (TYPES[g[0]], g[1])),
    (re.compile(r"(resize_fwd|resize_bwd|maxpool2_relu_bwd)_kernel" + RS_T + "E"), lambda g: "%s_kernel<%s>" % (g[0], TYPES[g[1]])),
]
REPORT_ONLY = ", scalar"                            # resample, views: kernels whose label holds this are reported, not held to the counts
HELD_SCALAR = "axpby_kernel<f32, scalar>"           # views: the one scalar form the product runs (the trainers' flat fp32 gradient sums)
VIEWS = False
VIEW_PAIRS = ("lrelu_bwd", "axpby", "l1_views", "nchw_to_nhwc")      # old: x_kernel / x_vec_kernel (l1_views: x_partial_kernel / x_vec_partial_kernel)
VIEW_SCALAR_ONLY = ("clamp_grad_kernel", "nhwc_to_nchw_kernel", "l1_grad_views_kernel")
VIEW_RENAMED = {"clamp_grad_rgb16_kernel": "rgb_to_nhwc_kernel<%s, CLAMP=1, WIDE=1>", "clamp_grad_rgb4_kernel": "rgb_to_nhwc_kernel<%s, CLAMP=1, WIDE=0>",
                "nchw_to_nhwc4_kernel": "rgb_to_nhwc_kernel<%s, CLAMP=0, WIDE=0>", "finish_sum_kernel": "finish_kernel<FinAxpy>",
                "finish_mean_kernel": "finish_kernel<FinMean>", "finish_sigmoid_mean_kernel": "finish_kernel<FinSigmoidMean>",
                "sn_dot_finish_kernel": "finish_kernel<SnDotFin>"}
VIEW_SYM = re.compile(r"_ZN7srganfd\d+?([a-z][a-z0-9_]*_kernel)(?:I(t|DF16_|f)((?:L[ib]\d+E)*)E|INS_\d+([A-Za-z]+)EE)?E")


def views_label(sym):
    """one label for a kernel of elementwise / loss / layout / norm .hip on either side of the refactor"""
    m = VIEW_SYM.match(sym)
    if not m:
        return None
    name, t, args, epi = m.groups()
    if epi:
        return "%s<%s>" % (name, epi)
    if name in VIEW_RENAMED:
        return VIEW_RENAMED[name] % TYPES[t] if "%s" in VIEW_RENAMED[name] else VIEW_RENAMED[name]
    if name == "rgb_to_nhwc_kernel":
        clamp, wide = re.findall(r"Lb(\d)E", args)
        return "rgb_to_nhwc_kernel<%s, CLAMP=%s, WIDE=%s>" % (TYPES[t], clamp, wide)
    for base in VIEW_PAIRS:
        tail = "_partial_kernel" if base == "l1_views" else "_kernel"
        if name == base + "_vec" + tail:
            return "%s%s<%s, vec>" % (base, tail, TYPES[t])
        if name == base + tail:
            n = re.findall(r"Li(\d+)E", args)
            return "%s%s<%s, %s>" % (base, tail, TYPES[t], "vec" if n and n[0] != "1" else "scalar")
    if name in VIEW_SCALAR_ONLY:
        return "%s<%s, scalar>" % (name, TYPES[t])
    return "%s<%s>" % (name, TYPES[t]) if t else name
TYPES = {"t": "bf16", "DF16_": "f16", "f": "f32"}
CLASSES = [("mfma", r"v_mfma"), ("lds", r"ds_"), ("global", r"(global|flat|scratch)_"), ("buffer", r"buffer_"), ("s_waitcnt", r"s_waitcnt"),
           ("s_barrier", r"s_barrier")]
DEGRADE_CLASSES = [("global load", r"(global|flat)_load"), ("global store", r"(global|flat)_store"), ("global atomic", r"(global|flat)_atomic"),
                   ("lds read", r"ds_read"), ("lds write", r"ds_write"), ("lds other", r"ds_"), ("scratch", r"scratch_"), ("scalar load", r"s_load|s_buffer_load"),
                   ("s_waitcnt", r"s_waitcnt"), ("s_barrier", r"s_barrier")]
DEGRADE_NAME = re.compile(r"_ZN7srganfd\d+?([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]\d+E)+)E)?E")
LISTED = []                                         # classes that are counted and listed where they moved, not held
AT_MOST = []                                        # classes whose count may fall but not rise
WAVE_STEPS = [64, 72, 80, 96, 128, 168, 256, 512]   # VGPRs per lane at which one more wave per SIMD is lost (512 registers, granule 8)


def waves(v):
    return 8 - next(i for i, s in enumerate(WAVE_STEPS) if v <= s)


def report_only(n):
    return REPORT_ONLY in n and n != HELD_SCALAR


def label(sym):
    for pat, fmt in RS_NAMES:
        m = pat.search(sym)
        if m:
            return fmt(m.groups()), None
    if VIEWS and views_label(sym):
        return views_label(sym), None
    if LISTED and DEGRADE_NAME.match(sym):
        name, args = DEGRADE_NAME.match(sym).groups()
        vals = ["true" if k == "b" and v == "1" else "false" if k == "b" else v for k, v in re.findall(r"L([ib])(\d+)E", args or "")]
        return name + ("<%s>" % ", ".join(vals) if vals else ""), None
    m = DC_NAME.search(sym)
    if m:
        return "dense_chain_kernel<%s, RPW=%s>" % (TYPES[m.group(1)], m.group(2)), None
    m = THIN_NAME.search(sym)
    if m:
        extra = ", MASK=%s, NT=%s" % (m.group(3), m.group(4)) if m.group(3) is not None else ""
        return "%s_kernel<%s%s>" % (m.group(1), TYPES[m.group(2)], extra), None
    if "thin_wgrad_reduce_kernel" in sym:
        return "thin_wgrad_reduce_kernel", None
    m = NAME.search(sym)
    if not m:
        return sym, None
    t, ks, st, xp, yp, dma, var = m.groups()
    return "wgrad_kernel<%s, KS=%s, STRIDE=%s, XP=%s, YP=%s, DMA=%s>" % (TYPES[t], ks, st, xp, yp, dma), var


def parse(path):
    out, cur, body, meta, in_meta = {}, None, [], [], False
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_ZN7srganfd\w+):", line)
        if m:
            cur, body, meta = m.group(1), [], []
            continue
        if cur is None:
            continue
        if s.startswith(".amdhsa_kernel "):
            in_meta = True
            continue
        if s == ".end_amdhsa_kernel":
            name, var = label(cur)
            ops = [re.sub(r"\s*;.*$", "", b).replace(cur, "@") for b in body]
            ops = [re.sub(r"\.LBB\d+_", ".LBB_", o) for o in ops]
            md = dict(x.split(None, 1) for x in meta)
            out[name] = dict(var=var, ops=ops, meta=md)
            cur, in_meta = None, False
            continue
        if in_meta:
            meta.append(s)
        elif s and not s.startswith((".", ";")) and not s.endswith(":"):
            body.append(s)
    return out


def counts(ops):
    c = collections.OrderedDict((k, 0) for k, _ in CLASSES)
    for o in ops:
        for k, pat in CLASSES:
            if re.match(pat, o):
                c[k] += 1
                break
    return c


def res(md):
    return "vgpr %s sgpr %s scratch %s lds %s kernarg %s" % (md[".amdhsa_next_free_vgpr"], md[".amdhsa_next_free_sgpr"],
                                                          md[".amdhsa_private_segment_fixed_size"], md[".amdhsa_group_segment_fixed_size"],
                                                          md[".amdhsa_kernarg_size"])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--kernel"]:
        if argv[1] in ("dense_chain", "thin"):
            CLASSES.append(("lane spills", r"v_(readlane|writelane)"))
            AT_MOST.append("lane spills")
        elif argv[1] == "views":
            global VIEWS
            VIEWS = True
        elif argv[1] == "degrade":
            CLASSES[:] = DEGRADE_CLASSES
            LISTED.extend(["scalar load", "s_waitcnt"])
        elif argv[1] not in ("wgrad", "resample"):
            sys.exit("--kernel: wgrad, dense_chain, thin, resample, views or degrade, not %r" % argv[1])
        argv = argv[2:]
    P, B = parse(argv[0]), parse(argv[1])
    only_p, only_b = sorted(set(P) - set(B)), sorted(set(B) - set(P))
    print("# parent: %d kernels, branch: %d kernels; only in parent: %d, only in branch: %d" % (len(P), len(B), len(only_p), len(only_b)))
    for n in only_p:
        print("only in parent: %s (VAR %s): %s" % (n, P[n]["var"], res(P[n]["meta"])))
    for n in only_b:
        print("only in branch: %s: %s" % (n, res(B[n]["meta"])))
    print("# per kernel: instruction stream / .amdhsa_kernel block (kernarg size aside) / resources parent | branch")
    bad, moved = [], []
    n_same, n_meta = 0, 0
    for n in sorted(set(P) & set(B)):
        p, b = P[n], B[n]
        same = p["ops"] == b["ops"]
        mp = {k: v for k, v in p["meta"].items() if k != ".amdhsa_kernarg_size"}
        mb = {k: v for k, v in b["meta"].items() if k != ".amdhsa_kernarg_size"}
        msame = mp == mb
        n_same += same
        n_meta += msame
        var = " (parent VAR %s)" % p["var"] if p["var"] is not None else ""
        print("%s%s: stream %s, metadata %s, %s | %s" % (n, var, "identical" if same else "DIFFERS", "identical" if msame else "DIFFERS",
                                                         res(p["meta"]), res(b["meta"])))
        cp, cb = counts(p["ops"]), counts(b["ops"])
        vp, vb = int(p["meta"][".amdhsa_next_free_vgpr"]), int(b["meta"][".amdhsa_next_free_vgpr"])
        sp, sb = int(p["meta"][".amdhsa_private_segment_fixed_size"]), int(b["meta"][".amdhsa_private_segment_fixed_size"])
        wv = [sum("vmcnt" in o for o in x["ops"] if o.startswith("s_waitcnt")) for x in (p, b)]
        waits_moved = VIEWS and cp["s_waitcnt"] != cb["s_waitcnt"] and wv[0] == wv[1]      # scalar (kernel-argument) waits alone: listed
        if report_only(n):
            print("    a scalar form: reported, not held to the parent's counts")
        elif any(cb[k] > cp[k] if k in AT_MOST else cb[k] != cp[k] for k in cp if not (waits_moved and k == "s_waitcnt") and k not in LISTED):
            bad.append(n + ": instruction-class counts differ")
        if LISTED:
            if p["meta"][".amdhsa_group_segment_fixed_size"] != b["meta"][".amdhsa_group_segment_fixed_size"]:
                bad.append(n + ": LDS bytes differ")
            moved.extend("%s: %s %d -> %d" % (n, k, cp[k], cb[k]) for k in LISTED if cp[k] != cb[k])
        if waits_moved and not report_only(n):
            moved.append("%s: s_waitcnt %d -> %d, those on vector memory %d on both sides" % (n, cp["s_waitcnt"], cb["s_waitcnt"], wv[0]))
        if sb > sp:
            bad.append(n + ": gains scratch")
        if waves(vb) < waves(vp) and not report_only(n):
            bad.append(n + ": crosses a wave-occupancy step (%d -> %d VGPRs)" % (vp, vb))
        if "DMA=1" in n and vb > 128 and vb > vp:
            bad.append(n + ": loader-wave kernel above 128 VGPRs")
        if not same:
            print("    instructions %d | %d" % (len(p["ops"]), len(b["ops"])))
            for k in cp:
                print("    %s %d | %d" % (k, cp[k], cb[k]))
            if cp["s_waitcnt"] != cb["s_waitcnt"]:      # which waits moved: those on vector memory, or those on scalar (kernel-argument) loads alone
                print("    s_waitcnt with vmcnt %d | %d, without (scalar loads, LDS) %d | %d" % (wv[0], wv[1], cp["s_waitcnt"] - wv[0], cb["s_waitcnt"] - wv[1]))
            op, ob = collections.Counter(o.split()[0] for o in p["ops"]), collections.Counter(o.split()[0] for o in b["ops"])
            print("    per opcode (differing only): " + ", ".join("%s %d|%d" % (k, op[k], ob[k]) for k in sorted(set(op) | set(ob)) if op[k] != ob[k]))
    print("# identical streams: %d of %d; identical metadata (kernarg size aside): %d of %d" % (n_same, len(set(P) & set(B)), n_meta, len(set(P) & set(B))))
    if LISTED:
        print("# scalar-load and s_waitcnt counts that moved (listed, not held): %d" % len(moved))
        for x in moved:
            print("#   " + x)
    if VIEWS:
        print("# s_waitcnt counts that moved with the kernel-argument layout (waits on vector memory equal): %d" % len(moved))
        for x in moved:
            print("#   " + x)
    print("# requirements not met: %d" % len(bad))
    for x in bad:
        print("#   " + x)


if __name__ == "__main__":
    main()

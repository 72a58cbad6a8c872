#!/usr/bin/env python3
"""Where do a GEMM kernel's cycles go?  Runs one problem through the DIAGNOSTIC library (make -C vae-los-angeles_amd/csrc STAMP=1
-> libmmvae_stamp.so, selected via MMVAE_LIB_PATH) whose kernels stamp cycle counters at the phases of every K / batch step (slot
layouts: common.h), and prints cycles per step:

    python tools/stamp.py KERNEL [N K M]

    nt    first-generation NT kernel (gemm_nt.hip), 128x256 and 128x128 tiles; SRC=f32: fp32 A, STATS=1: column statistics
    nt2   second-generation NT kernel (gemm_nt2.h), plain bf16 A; STATS=1 as above
    ntp   wave-specialised NT kernel (gemm_ntp.h), fp32 A; PRO=1: bf16 A through the BatchNorm + ReLU + Dropout prologue
    tn    128x128 TN (dW) kernel (gemm_tn.hip), register-staged form: M not a multiple of 64 (the LDS-DMA form has no step stamps)
    tnw   wide-tile dW kernel (gemm_tn_wide.hip), BatchNorm-corrected bf16 P and fp32 Q (EncoderB.L0.dW); PLAIN=1: plain bf16 P
          and Q (such a problem only goes there with N * K >= 4M)
    loss  the decoder-final GEMMs with their loss epilogue (nt2 kernel): two fixed layer shapes, N and K are ignored

nt and nt2 switch the kernels that would otherwise take their problem off (mmvae_set_tuning keys 8 and 2).
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["MMVAE_LIB_PATH"] = os.path.join(ROOT, "vae-los-angeles_amd", "mmvae", "libmmvae_stamp.so")
sys.path[:0] = [os.path.join(ROOT, "vae-los-angeles_amd")]
import torch  # noqa: E402
from mmvae import _lib as L, ops  # noqa: E402
from mmvae.ops import PREC_BF16  # noqa: E402

STAMP_NT, STAMP_NT2, STAMP_NTP, STAMP_TN, STAMP_TNW = range(5)      # common.h
dev, REPS = "cuda", 5
lib = L.load()
lib.mmvae_debug_stamps.argtypes = [C.c_int32, C.POINTER(C.c_uint64), C.c_int32, C.c_int32]
env = os.environ.get


def measure(kernel, fn, warm=2, steps=4):
    """(slots, us per call) of REPS timed calls fn(i), after `warm` calls whose stamps are dropped; slot `steps` counts the steps"""
    buf = (C.c_uint64 * 16)()
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    L.check(lib.mmvae_debug_stamps(kernel, buf, 16, 1), "mmvae_debug_stamps")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REPS):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    L.check(lib.mmvae_debug_stamps(kernel, buf, 16, 1), "mmvae_debug_stamps")
    s = [int(x) for x in buf]
    if not s[steps]:
        sys.exit(f"no stamped steps: the problem ran on another kernel or form than the one asked for (id {kernel})")
    return s, e0.elapsed_time(e1) * 1e3 / REPS


def prepared(N, K):
    pl = ops.PreparedLinear([torch.randn(N, K, device=dev) / 30], [torch.zeros(N, device=dev)], PREC_BF16, dev)
    ops.WeightPrep([pl], dev).run()
    return pl


def nt(N, K, M, kernel):
    f32 = kernel == STAMP_NT and env("SRC") == "f32"
    A = [torch.randn(M, K, device=dev) if f32 else torch.randn(M, K, device=dev).bfloat16() for _ in range(3)]
    stats = torch.zeros(2, N, dtype=torch.float64, device=dev) if env("STATS") == "1" else None
    pl = prepared(N, K)
    out = torch.empty(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
    lib.mmvae_set_tuning(8, 0)
    lib.mmvae_set_tuning(2, 0 if kernel == STAMP_NT else 1)
    names = ["reads(s1) + mma(s0) issue", "stage: vmcnt wait + ds_write + drain", "barrier wait", "fetch + reads(s0) + mma(s1) issue"]
    if kernel == STAMP_NT2:
        names = ["wait for the own DMA (vmcnt)", "barrier wait", "DMA issue of the next step", "fragment reads + 32 MFMA"]
    for wide in (1, 0):
        lib.mmvae_set_tuning(0, 0 if wide else 1 << 30)
        s, us = measure(kernel, lambda i: ops.gemm_nt(PREC_BF16, A[i % 3], pl.w, N, K, out, bias=pl.bias, stats=stats))
        steps, waves = s[4], s[5]
        print(f"N={N} K={K} M={M} {'wide 128x256' if wide else 'narrow 128x128'}: {us:.1f} us/launch (stamped build), {waves // REPS} waves, {steps // waves} K steps/wave")
        tot = sum(s[:4])
        for nm, v in zip(names, s[:4]):
            print(f"   {nm:40s} {v / steps:8.1f} cycles/K-step  {100.0 * v / tot:5.1f} %")
        print(f"   {'  of stage: wait for the global loads':40s} {s[7] / steps:8.1f} cycles/K-step")
        print(f"   {'sum':40s} {tot / steps:8.1f} cycles/K-step;  whole kernel {s[6] / waves:9.0f} cycles/wave, main loop {tot / waves:9.0f}, before it {s[8] / waves:7.0f}, epilogue {s[9] / waves:7.0f}")


def ntp(N, K, M):
    pro_on = env("PRO") == "1"      # bf16 A through the producers' BatchNorm + ReLU + Dropout prologue (EncoderB's second Linear: N=256 K=512)
    A = [torch.randn(M, K, device=dev).bfloat16() if pro_on else torch.rand(M, K, device=dev) for _ in range(3)]
    pro = (torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev) * 0.3, (torch.rand(M, K, device=dev) > 0.1).to(torch.uint8), 1.0 / 0.9) if pro_on else None
    stats = torch.zeros(2, N, dtype=torch.float64, device=dev)
    pl = prepared(N, K)
    out = torch.empty(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
    s, us = measure(STAMP_NTP, lambda i: ops.gemm_nt(PREC_BF16, A[i % 3], pl.w, N, K, out, bias=pl.bias, stats=stats, prologue=pro), steps=3)
    wgs = max(s[6], 1)
    steps, tiles = s[3] / wgs, s[4] / wgs
    print(f"N={N} K={K} M={M}: {us:.1f} us/launch (stamped build); per sampled workgroup: {steps:.0f} K steps, {tiles:.0f} tiles, "
          f"{s[5] / wgs:.0f} cycles in the kernel")
    print(f"  consumer   : barrier wait {s[0] / wgs / steps:7.0f} /step   reads+MFMA {s[1] / wgs / steps:7.0f} /step   epilogue {s[2] / wgs / max(tiles, 1):7.0f} /tile")
    names = ["barrier wait", "wait for the set's loads", "v_cvt_pk (fp32 -> bf16)", "ds_write issue", "W DMA issue", "A load issue", "wait for W of the next step"]
    print("  producer   : " + "   ".join(f"{n} {s[8 + i] / wgs / steps:6.0f}" for i, n in enumerate(names)) + "   (cycles per K step)")


def tn(N, K, M):
    P = [torch.randn(M, ops.ceil_to(N, 8), device=dev).bfloat16() for _ in range(3)]
    Q = [torch.randn(M, ops.ceil_to(K, 8), device=dev).bfloat16() for _ in range(3)]
    dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    slab = torch.empty(1 << 25, device=dev)            # as in the engine: partial tiles of the batch splits go to a slab workspace
    s, us = measure(STAMP_TN, lambda i: ops.gemm_tn(PREC_BF16, P[i % 3], Q[i % 3], dw, db, N, K, slab=slab))
    steps, waves = s[4], s[5]
    print(f"TN N={N} K={K} M={M}: {us:.1f} us/launch (stamped build), {waves // REPS} sampled waves, {steps // waves} batch steps/wave")
    names = ["fragment step 0 (tr reads + 16 MFMA)", "stage (vmcnt wait + ds_write)", "fragment step 1 + fetch issue + drain", "barrier wait"]
    tot = sum(s[:4])
    for nm, v in zip(names, s[:4]):
        print(f"   {nm:42s} {v / steps:8.1f} cycles/step  {100.0 * v / tot:5.1f} %")
    print(f"   {'  of stage: wait for the global loads':42s} {s[7] / steps:8.1f} cycles/step")
    print(f"   sum {tot / steps:8.1f} cycles/step; whole kernel {s[6] / waves:9.0f} cycles/wave, loop {tot / waves:9.0f}, before {s[8] / waves:7.0f}, after {s[9] / waves:7.0f}")


def tnw(N, K, M):
    kind = "plain" if env("PLAIN") == "1" else "bn"
    slab = torch.empty(1 << 25, device=dev)
    Np, Kp = ops.ceil_to(N, 8), ops.ceil_to(K, 8)
    P = [torch.randn(M, Np, device=dev).bfloat16() for _ in range(3)]
    dw = torch.zeros(N, K, device=dev); db = torch.zeros(N, device=dev)
    if kind == "bn":
        Y = [torch.randn(M, Np, device=dev).bfloat16() for _ in range(3)]
        Q = [torch.randn(M, K, device=dev) for _ in range(3)]
        mean, rstd = torch.randn(N, device=dev) * 0.1, torch.rand(N, device=dev) + 0.5
        coef = torch.stack([torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev) * 0.01, torch.randn(N, device=dev) * 0.01]).contiguous()
        def f(i): ops.gemm_tn(PREC_BF16, P[i % 3], Q[i % 3], dw, db, N, K, p_prologue=(Y[i % 3], mean, rstd, coef), slab=slab)
    else:
        Q = [torch.randn(M, Kp, device=dev).bfloat16() for _ in range(3)]
        def f(i): ops.gemm_tn(PREC_BF16, P[i % 3], Q[i % 3], dw, db, N, K, slab=slab)
    s, us = measure(STAMP_TNW, f, warm=3)
    steps, wgs = s[4], s[5]
    print(f"{kind} N={N} K={K} M={M}: {us:.1f} us/call incl. reduce (stamped build); {wgs // REPS} stamped workgroups, {steps // max(wgs, 1)} steps each")
    print(f"   whole kernel {s[6] / max(wgs, 1):9.0f} cycles per workgroup, epilogue {s[7] / max(wgs, 1):8.0f}")
    tot = sum(s[:4])
    for nm, v in zip(["wait for the own DMA (vmcnt)", "barrier", "DMA issue", "fragments + MFMA"], s[:4]):
        print(f"   {nm:32s} {v / max(steps, 1):8.1f} cycles/step {100.0 * v / max(tot, 1):5.1f} %")


def loss(N_, K_, M):
    for name, N, K, bce in (("DecoderB.L2 572<-512 BCE", 572, 512, True), ("DecoderA.L1 782<-128 MSE", 782, 128, False)):
        A = [torch.randn(M, K, device=dev).bfloat16() for _ in range(3)]
        W = torch.randn(N, K, device=dev) / K ** 0.5
        pl = ops.PreparedLinear([W], [torch.zeros(N, device=dev)], PREC_BF16, dev); ops.WeightPrep([pl], dev).run()
        T = [torch.rand(M, N, device=dev) for _ in range(3)]
        g = torch.empty(M, ops.ceil_to(N, 8), dtype=torch.bfloat16, device=dev)
        sums = torch.zeros(5, dtype=torch.float64, device=dev)
        s, us = measure(STAMP_NT2, lambda i: ops.gemm_nt(PREC_BF16, A[i % 3], pl.w, N, K, g, bias=pl.bias, epilogue=ops.EPI_LOSS_BCE_LOGIT if bce else ops.EPI_LOSS_MSE,
                                                         h=T[i % 3], loss_sum=sums[1:2] if bce else sums[0:1]))
        steps, waves = s[4], s[5]
        tiles = steps / ((K + 63) // 64)
        print(f"{name}: {us:.1f} us/launch (stamped); {waves // REPS} sampled waves, {steps / waves:.0f} K steps, {tiles / waves:.1f} tiles per wave")
        for nm, v in zip(["wait for the own DMA", "barrier wait", "DMA issue of the next step", "fragment reads + 32 MFMA"], s[:4]):
            print(f"   {nm:32s} {v / steps:8.0f} cycles/K-step")
        print(f"   whole kernel {s[6] / waves:9.0f} cycles/wave: main loop {sum(s[:4]) / waves:9.0f}, epilogues {s[9] / waves:9.0f} = {s[9] / tiles:7.0f} per tile")


# kernel -> (default N K M, run)
KERNELS = {
    "nt": ((512, 1024, 65536), lambda N, K, M: nt(N, K, M, STAMP_NT)),
    "nt2": ((512, 1024, 65536), lambda N, K, M: nt(N, K, M, STAMP_NT2)),
    "ntp": ((512, 572, 65536), ntp),
    "tn": ((572, 512, 65000), tn),
    "tnw": ((512, 572, 65536), tnw),
    "loss": ((0, 0, 65536), loss),
}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in KERNELS:
        sys.exit(__doc__)
    shape, run = KERNELS[sys.argv[1]]
    run(*[int(a) for a in sys.argv[2:5]], *shape[len(sys.argv[2:5]):])

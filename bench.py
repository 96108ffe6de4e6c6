#!/usr/bin/env python3
"""Benchmark of the w-OFDM Monte-Carlo BER hot path on MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1], SURVEY.md 8d "C2"): wtx-OFDM, N=256, 16-QAM, CP=32/CS=8,
raised-cosine windows, Veh-A channel fixture #0, 12 SNR points -5:5:50 dB.  One *step* = one
pass of the hot path: 62,500 frames (1e6 OFDM symbols) at each of the 12 SNR points per GPU,
fresh random data every step (global frame index keys the Philox streams), followed by the
all-reduce of the error counters.  Weak scaling: every rank simulates its own 62,500 frames per
cell per step.  value = OFDM symbols (pilot included) simulated by all ranks / wall time.

A plain run sets up, warms up, times --steps steps and prints the line.  --full adds the CPU
baseline legs (the oracle timed on a sample of the same workload) and the BER check against the
oracle on the same frames (`cpu_baseline`, `ber_vs_reference`).  --dump-outputs DIR writes the
counters of the timed sweep and their BER as DIR/counts.npy and DIR/ber.npy (float64); the inputs
depend on the arguments only, so two builds can be compared output for output.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3          # MI355X_MICROARCH.md: fp32 vector peak (= fp32 MFMA dense peak)
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense f16 / bf16 matrix peak (no sparsity)
FRAMES_PER_STEP = 62500           # x 16 symbols = 1e6 OFDM symbols per SNR point
SNR_DB = np.arange(-5.0, 51.0, 5.0)


def f_sym(st, n_taps):
    """Algorithmic flop per OFDM symbol, SURVEY.md 8(d)."""
    N, P, B = st.n_fft, st.sym_len, st.stride
    return (2 * 5 * N * int(np.log2(N)) + 8 * n_taps * B + 2 * P + 2 * st.tail_tx + 10 * B
            + 2 * (N + st.tail_rx) + 2 * st.tail_rx + 11 * N)


def cpu_baseline(W, st, w_tx, w_rx, h, seed, target_s=10.0, dense_s=8.0):
    """The oracle (CPU port of the reference algorithm, fp64, OpenMP over frames) timed on a bounded
    sample of the same workload, frames [0, Fs) of every SNR cell, in two cost structures:
      value     FFT form: Tx / Rx as N log N transforms (the fastest faithful CPU formulation);
      faithful  the reference's own formulation: the hoisted dense operators tx_mat [P x N] and rx_mat
                [N x B] applied as matrix products in every frame (wofdm_simulation.py:464-471, 187-222)."""
    from oracle import oracle as O
    osys = O.make_sys(st.n_fft, 4, 16, st.cp, st.cs, st.tail_tx, st.tail_rx, st.prefix_rm,
                      st.circ_shift, h.shape[1], 1)
    args = (osys, w_tx.astype(np.float64), w_rx.astype(np.float64), h.astype(np.complex128),
            SNR_DB, seed)
    # the threads we may really use: the process's CPU affinity (the GPU box exposes many more
    # hardware threads than its CPU share), capped by OpenMP's own limit
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(O.threads(), avail, int(os.environ.get("WOFDM_CPU_THREADS", "64"))))

    def leg(dense, budget_s):
        O.run(*args, 0, 2 * threads, n_threads=threads, dense=dense)   # warm-up (thread pool, page faults)
        t0 = time.perf_counter()
        O.run(*args, 0, 4 * threads, n_threads=threads, dense=dense)
        rate = 4 * threads / (time.perf_counter() - t0)                # frames per cell per second
        frames = int(max(4 * threads, min(60000, rate * budget_s)))
        t0 = time.perf_counter()
        counts = O.run(*args, 0, frames, n_threads=threads, dense=dense)
        dt = time.perf_counter() - t0
        return frames, counts, frames * 16 * SNR_DB.size, dt

    frames, counts, syms, dt = leg(False, target_s)
    dframes, dcounts, dsyms, ddt = leg(True, dense_s)
    dsame = bool(np.array_equal(dcounts, O.run(*args, 0, dframes, n_threads=threads)))
    return dict(value=syms / dt, unit="OFDM symbols/s", cores=threads, kind="port",
                sample="frames [0,%d) of each of the %d SNR cells = %d symbols in %.1f s; "
                       "oracle/wofdm_oracle.c, fp64, OpenMP over frames, FFT form" % (frames, SNR_DB.size, syms, dt),
                faithful=dict(value=dsyms / ddt, unit="OFDM symbols/s", cores=threads,
                              sample="frames [0,%d) of each cell = %d symbols in %.1f s; the reference's dense "
                                     "tx_mat / rx_mat products per frame (wofdm_simulation.py:464-471); counters "
                                     "%s the FFT form's" % (dframes, dsyms, ddt, "equal" if dsame else "DIFFER from")),
                ), frames, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    # everything beyond the headline figure: the CPU baseline legs and the BER check against the oracle
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")    # with --full: skip those extras again
    # after the timed steps: write the counters the last timed step left (and their BER) as DIR/<name>.npy
    ap.add_argument("--dump-outputs", metavar="DIR")
    ap.add_argument("--frames-per-step", type=int, default=FRAMES_PER_STEP)
    # first frame of the run (per cell): lets a one-rank run cover exactly the frames an N-rank run covered (bit-identical counters)
    ap.add_argument("--frame-offset", type=int, default=0)
    # rehearsal of the N>1 code path on a one-GPU box: all ranks on cuda:0, gloo collectives
    ap.add_argument("--rehearse-on-one-gpu", action="store_true")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist
    import wofdm_amd as W

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run)"
                         % (a.gpus, world))
    if a.rehearse_on_one_gpu:
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.rehearse_on_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    seed = 2
    st = W.make_structure("wtx", 256, 32)
    w_tx = W.tx_rc_window(st).astype(np.float32)
    w_rx = W.rx_rc_window(st).astype(np.float32)
    h = np.load(os.path.join(ROOT, "tests", "golden", "channels_vehA.npz"))["h"][:1].astype(np.complex64)
    cfg = W.make_cfg(st, 4, 16, h.shape[1], 1, SNR_DB.size, 1, noise_before_truncate=True, seed=seed)
    plan = W.Plan(cfg, w_tx, w_rx, h, SNR_DB.astype(np.float32), device=local)
    F = a.frames_per_step
    counts = plan.new_counts()
    stream = torch.cuda.current_stream()

    def step(i):
        # rank r simulates frames [(i*world + r)*F, +F) of every cell
        plan.launch(a.frame_offset + (i * world + rank) * F, F, counts, stream)
        reduce_counts()

    def reduce_counts():
        # device tensor: reduced in place by RCCL under "nccl", through a host copy under "gloo"
        W.distributed.all_reduce_counts(counts)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(a.warmup):
        step(i)
    if world > 1 and a.warmup == 0:
        # communicator set-up (lazy in RCCL) must not land in the timed region
        reduce_counts()
    fence()
    counts.zero_()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(a.steps)]
    fence()
    t0 = time.perf_counter()
    for i in range(a.steps):
        ev[i][0].record(stream)
        plan.launch(a.frame_offset + (a.warmup + i) * world * F + rank * F, F, counts, stream)
        ev[i][1].record(stream)
        # counters are running sums, so reducing inside the loop would multiply-count; the
        # reduce of the sweep's counters happens once, below, inside the timed region
    reduce_counts()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if a.rehearse_on_one_gpu else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    kern_ms = [e0.elapsed_time(e1) for e0, e1 in ev]

    syms_per_launch = F * 16 * SNR_DB.size
    total_syms = syms_per_launch * a.steps * world
    fs = f_sym(st, h.shape[1])
    avg_ms = float(np.mean(kern_ms))
    achieved = syms_per_launch * fs / (avg_ms * 1e-3) / 1e12
    host = counts.cpu().numpy().view(np.uint64)
    ber = (host[0, :, 0, 0] / np.maximum(host[0, :, 0, 1], 1)).tolist()

    if rank == 0:
        # HBM bytes per launch come from rocprofv3 PMC passes (not collectable from inside this run):
        # the committed figure is used only while it was measured on exactly these kernel sources
        traffic, pipes = None, None
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("kernel_source_hash") == W.kernel_source_hash():
                    traffic = tj.get("bytes_per_launch")
                    # What the two pipes actually ISSUE (PMC counts of the same launch x this run's launch rate): the
                    # algorithmic figure above charges the FIR's fp32 flop although it executes as f16 MFMAs.
                    vi, mi = tj.get("valu_insts_per_launch"), tj.get("mfma_insts_per_launch")
                    va, ga = tj.get("valu_active_quadcycles_per_launch"), tj.get("gui_active_cycles_per_launch")
                    if vi and mi:
                        per_s = 1.0 / (avg_ms * 1e-3)
                        simds = 1024
                        pipes = {
                            "valu": {"wave_insts_per_symbol": vi / syms_per_launch,
                                     "busy_frac": (va / (ga / 8.0 * simds / 4.0)) if va and ga else None},
                            "mfma_f16": {"insts_per_symbol": mi / syms_per_launch, "tflops": mi * 16 * 16 * 32 * 2 * per_s / 1e12,
                                         "peak_tflops": PEAK_F16_MFMA_TFLOPS,
                                         "frac": mi * 16 * 16 * 32 * 2 * per_s / 1e12 / PEAK_F16_MFMA_TFLOPS},
                            "note": "issued work per pipe, from rocprofv3 PMC counts of this kernel on these sources "
                                    "(profiles/hbm_traffic.json): valu.busy_frac = SQ_ACTIVE_INST_VALU quad-cycles over the "
                                    "launch's SIMD quad-cycles (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs / 4) as profiled; "
                                    "mfma_f16 = v_mfma_f32_16x16x32_f16 flop at this run's launch rate against the dense "
                                    "f16 matrix peak"}
            except Exception:
                traffic, pipes = None, None
        out = {
            "metric": "OFDM symbols/sec (whole node) + BER vs reference, N=256 16-QAM",
            "value": total_syms / dt, "unit": "OFDM symbols/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "C2: wtx-OFDM N=256 16-QAM CP=32 CS=8 RC windows, 21-tap Veh-A "
                                   "fixture #0, 12 SNR points -5:5:50 dB, %d frames x 16 symbols per SNR "
                                   "point per GPU per step, Philox4x32-10 on device" % F,
                       "frames_per_cell_per_step": F, "cells": int(SNR_DB.size),
                       "symbols_per_step_per_gpu": syms_per_launch, "parallelism": "frames/%d" % world},
            "roofline": {"bound": "valu", "achieved": achieved, "peak": PEAK_FP32_TFLOPS,
                         "unit": "TFLOP/s", "frac": achieved / PEAK_FP32_TFLOPS, "traffic": traffic,
                         "kernel": "wofdm_frames_kernel<256,4,%d,false,false,0>" % plan.kernel_id()[0],
                         "kernel_ms_avg": avg_ms, "pipes": pipes,
                         "flop_per_symbol": fs,
                         "note": "achieved = algorithmic fp32 flop (SURVEY.md 8d F_sym x symbols) / kernel time, "
                                 "against the fp32 vector peak 157.3 TFLOP/s (= the fp32 MFMA dense peak). VALU issue "
                                 "is the binding pipe (RNG, mapping, window and f16-split work); the 21-tap FIR -- 64 % "
                                 "of F_sym -- and both 256-point transforms -- 27 % -- run on the matrix pipe as 3-term "
                                 "f16-split products with fp32 accumulation (block-Toeplitz FIR, two 16x16 DFT stages). "
                                 "HBM is not the bound: generate mode reads constants and writes counters only "
                                 "(traffic = PMC bytes per launch, null when not measured on these sources)."},
            "ber": ber, "snr_db": SNR_DB.tolist(),
            "bit_errors": [int(x) for x in host[0, :, 0, 0]], "bits": [int(x) for x in host[0, :, 0, 1]],
        }
        if a.dump_outputs:
            # what a caller of the timed path holds after its last step: the counter tensor
            # [pairs][snr][channels][bit errors, bits, symbol errors, symbols] (running sums over the timed
            # steps, reduced over the ranks) and the BER per SNR point; float64 keeps the counts exact
            os.makedirs(a.dump_outputs, exist_ok=True)
            np.save(os.path.join(a.dump_outputs, "counts.npy"), host.astype(np.float64))
            np.save(os.path.join(a.dump_outputs, "ber.npy"), np.asarray(ber, dtype=np.float64))
        if a.full and not a.no_cpu_baseline and world == 1:       # CPU leg: rank 0 at N=1 only
            base, fsamp, ocounts = cpu_baseline(W, st, w_tx, w_rx, h, seed)
            out["cpu_baseline"] = base
            # BER vs the reference algorithm on the very same frames (same Philox streams)
            g = plan.run(0, fsamp)
            o = ocounts
            gb = g[0, :, 0, 0] / g[0, :, 0, 1]
            ob = o[0, :, 0, 0] / o[0, :, 0, 1]
            out["ber_vs_reference"] = {
                "frames_per_cell": fsamp, "max_abs_ber_diff": float(np.abs(gb - ob).max()),
                "bit_error_count_diff": [int(x) for x in (g[0, :, 0, 0].astype(np.int64)
                                                         - o[0, :, 0, 0].astype(np.int64))],
                "bits_equal": bool(np.array_equal(g[..., 1], o[..., 1]))}
        print(json.dumps(out))
    plan.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""bench.py -- ORB extract + stereo match throughput on KITTI geometry (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--pairs P] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times exactly K steps once (no events inside them), writes the last step's outputs to DIR if
--dump-outputs is given (dump_outputs) and prints the line: metric, value (pairs/s), unit, ms_per_step, dtype, ... .  --full adds
everything else described below -- the timed region repeated (--repeat, --min-region-ms), the roofline with its per-stage table,
the pipelined / one-chain / strong-scaling passes, small batch, natural image, secondary configs, host-fed rate, the CPU baseline
and the post-run oracle spot check.

One process per GPU.  The driver launches N>1 through torch.distributed.run; started WITHOUT a launcher (`python bench.py --gpus N`, no
RANK / WORLD_SIZE in the environment) this process spawns the N ranks itself before anything touches the GPU and relays rank 0's line
(launch_ranks); a rank count that differs from --gpus is an error on every path, never a silent one-rank result.  A "step"
is one pass of the hot path (extract left + extract right + ComputeStereoMatches) over
one batch of P synthetic KITTI-geometry stereo pairs that are already resident in HBM.
Frame pairs are independent, so ranks shard them with no data-path collective; the only
RCCL traffic is a one-time broadcast of the extractor parameters, pattern checksum and a
(synthetic) fbow vocabulary from rank 0 at start-up.  Rank 0 prints ONE JSON line.

The headline timed region runs one step chain at a time (--chains 1): that keeps every kernel alone on the chip, so the
dominant kernel's HIP-event time, the rocprofv3 summary and `roofline` describe the kernel and not its neighbours.  Consecutive
steps are independent, though, and a deployment keeps several in flight: step k on context k % C and that context's stream, so
that one step's latency-bound stages (pyramid chain, quadtree, median) hide under another's issue-bound ones (FAST, describe).
That regime is timed right after the headline region with the same protocol and reported as config.pipelined (--pipelined C,
default 3; kernels of different chains share the chip there, so their individual durations stretch while throughput rises),
and for BASELINE config 4's 8 pairs per GPU as config.small_batch.  The timed region is repeated --repeat times (same --steps
each; --full: 5 by default, else once); `value` is the median, config.repeat holds min / max.

Two sharding modes (BASELINE.json config 4 = "64 frame pairs in flight, sharded across 8x"):
  --mode weak   (default, the headline `value`): P pairs per step PER GPU, "scaling": "weak";
  --mode strong : P pairs per step IN TOTAL, dealt round-robin by dist.shard_pairs (8 per GPU at N = 8),
                  "scaling": "strong".  A weak run on N > 1 GPUs also times a short strong pass and reports it
                  under config.strong_scaling, so one driver run shows both regimes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, NFEAT, NLEVELS = 1241, 376, 2000, 8
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448  # Config/Stereo-KITTI00-02.yaml
LEVEL_PX = [1241 * 376, 1034 * 313, 862 * 261, 718 * 218, 598 * 181, 499 * 151, 416 * 126, 346 * 105]
P_SUM = sum(LEVEL_PX)
# algorithmic bytes per image / per stereo pair (N = 2000)
B_PYR = sum(LEVEL_PX[:7]) + sum(LEVEL_PX[1:])
B_FAST = P_SUM
B_BLUR = 2 * P_SUM
B_DESC = NFEAT * (749 + 512 + 32 + 28)
B_IMG = B_PYR + B_FAST + B_BLUR + B_DESC
B_STEREO = 2 * NFEAT * 32 + NFEAT * (121 + 231) + NFEAT * 8
B_PAIR = 2 * B_IMG + B_STEREO
assert B_PAIR == 19_567_078, B_PAIR
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec


def stage_alg_bytes_per_pair(n_cand_per_image: float):
    """Algorithmic bytes per pair attributed to each stage."""
    return {
        "ingest": 2 * 2 * LEVEL_PX[0],
        "pyramid": 2 * B_PYR,
        "blur": 2 * B_BLUR,
        "fast": 2 * B_FAST,
        # not in SURVEY's formula (it prices pixels only): candidate records in, keypoint slots out
        "octree": 2 * (n_cand_per_image * 5 + NFEAT * 5),
        "describe": 2 * B_DESC,
        "stereo_match": B_STEREO,
        "stereo_median": NFEAT * 4 + NFEAT * 8,
    }


PROFILE_ROUND = "r05"
_STALE = []  # profile files whose build id is not the id of the library that ran (reported as roofline.stale_profiles)


def lib_build_id():
    try:
        from orbslam2_amd import api
        return api.build_id()
    except Exception:
        return None


def _profile_path(name):
    """profiles/<round>_<name> -- ONLY this round's file, and only when it carries the build id of the liborbfe.so this process
    has loaded (tools/collect_profiles.sh stamps every counter file with orbfe_build_id() of the build it profiled).  Counters of
    another build are not replayed: the field they would feed is null and the file is listed under roofline.stale_profiles."""
    path = os.path.join(ROOT, "profiles", "%s_%s" % (PROFILE_ROUND, name))
    if not os.path.exists(path):
        return None
    try:
        if path.endswith(".json"):
            have = json.load(open(path)).get("build_id")
        else:
            first = open(path).readline()
            have = first.split("build_id:")[1].strip() if "build_id:" in first else None
    except Exception:
        have = None
    if have is None or have != lib_build_id():
        if os.path.basename(path) not in _STALE:
            _STALE.append(os.path.basename(path))
        return None
    return path


def traffic_bytes(stage: str, pairs: int, launches: int):
    """HBM bytes per launch of the stage's kernel REPLAYED from this round's committed rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE collected in separate passes of this same command, gfx950 correction 2 x FETCH_SIZE as MI355X_MICROARCH.md
    prescribes), scaled from the profiled batch to this run's batch; None if not profiled or profiled on another build."""
    try:
        t = json.load(open(_profile_path("traffic.json")))["kernels"][stage]
        per_pair = (2.0 * t["fetch_kb_per_pair"] + t["write_kb_per_pair"]) * 1024.0
        return per_pair * pairs / launches
    except Exception:
        return None


def whole_step_traffic_per_pair():
    """Counter bytes (2 * FETCH_SIZE + WRITE_SIZE) * 1024 of every kernel of a step, per pair, from the same passes (decimal
    bytes, to be set against SURVEY's 19 567 078 algorithmic bytes); None if not profiled on this build.  The stereo matcher's
    descriptor gathers are counted by FETCH_SIZE as whole 64-byte sectors (tools/ubench/fetch_calib.hip), so its share is an upper bound."""
    try:
        path = _profile_path("traffic.json")
        ks = json.load(open(path))["kernels"]
        return sum((2.0 * t["fetch_kb_per_pair"] + t["write_kb_per_pair"]) * 1024.0 for t in ks.values()), os.path.basename(path)
    except Exception:
        return None, None


def _sq_valu_per_pair():
    """SQ_INSTS_VALU per stereo pair of every kernel of the step, from this round's rocprofv3 counter pass on this build (launches
    of 64 pairs; the counts file says how often a kernel ran per step): {kernel name fragment: wave-instructions per pair}."""
    path = _profile_path("pmc_sq.txt")
    if path is None:
        return None, None
    rows = []
    for line in open(path):
        if "SQ_INSTS_VALU" not in line or "{" not in line:
            continue
        d = eval(line[line.index("{"):line.rindex("}") + 1], {"__builtins__": {}})
        kern = line[:line.index("{")].strip()
        tail = line[line.rindex("}"):]
        n = int(tail[tail.index("n=") + 2:]) if "n=" in tail else 1
        if "rocclr" in kern or "candidates_gather" in kern:  # runtime copies; the parity tap of the post-run check
            continue
        rows.append((kern, d["SQ_INSTS_VALU"], n))
    # launches per step of a kernel = its dispatch count / fast_cell_kernel's (one per step)
    steps = max([n for k, _, n in rows if "fast_cell_kernel" in k] or [1])
    out = {}
    for kern, v, n in rows:
        out[kern] = out.get(kern, 0.0) + v * (n / steps) / 64.0
    return (out, os.path.basename(path)) if out else (None, None)


def valu_issue(pairs: int, launches: int, launch_ms: float, step_ms: float):
    """Context for the roofline: the path is bound by VALU issue, not by HBM.  SQ_INSTS_VALU from the committed rocprofv3 pass,
    scaled to this run's batch, against the issue rates MEASURED on this chip (profiles/r02_valu_peak.json, tools/ubench/valu_peak.hip,
    outside rocprofv3): gfx950 issues packed / integer min-max, v_perm, shifts, v_dot4, mbcnt ... once per ~4.1 cycles per SIMD
    (590 G wave-instructions/s chip-wide at the clock it holds) and add / sub / and / xor / mov / fp32 mul-add-fma once per ~2.3.
      frac       the dominant kernel's instructions priced as if ALL were half-rate (round 2's figure, an upper bound of the truth);
      frac_mix   priced by the kernel's opcode histogram (profiles/r03_isa_mix.json: tools/isa_mix.py disassembles the kernels, prices
                 every opcode with its measured cycles and weights each phase by its measured SQ_INSTS_VALU);
      whole_step the same two figures for the sum of every kernel of a step against the measured ms_per_step."""
    try:
        per_pair, src = _sq_valu_per_pair()
        ops = json.load(open(os.path.join(ROOT, "profiles", "r02_valu_peak.json")))["ops"]
        half_rate = ops["v_pk_max_i16"]["8"]["chip_G_wave_inst_per_s"] * 1e9   # the class FAST is made of (pk min / max, perm)
        full_rate = ops["v_add_u32"]["8"]["chip_G_wave_inst_per_s"] * 1e9      # add / sub / and / xor / mov / fp32 fma
        fast = next(v for k, v in per_pair.items() if "fast_cell_kernel" in k)
        insts = fast * pairs / launches
        out = {"wave_insts_per_launch": insts, "peak_wave_insts_per_s": half_rate, "frac": insts / (launch_ms * 1e-3) / half_rate, "counter_source": "profiles/" + src,
               "peak_source": "profiles/r02_valu_peak.json: v_pk_max_i16 at 8 waves per SIMD (measured, %.2f cycles per wave-instruction per SIMD); "
                              "full-rate class (v_add_u32 ...) %.0f G/s" % (ops["v_pk_max_i16"]["8"]["cycles_per_wave_inst_per_simd"], full_rate / 1e9)}
        total = sum(per_pair.values()) * pairs
        whole = {"wave_insts_per_step": total, "frac": total / (step_ms * 1e-3) / half_rate}
        mix_path = _profile_path("isa_mix.json")
        if mix_path:
            mix = json.load(open(mix_path))["kernels"]
            simd_cycles_per_s = half_rate * ops["v_pk_max_i16"]["8"]["cycles_per_wave_inst_per_simd"]  # 1024 SIMDs x the clock the chip held
            def seconds(n, kern):  # n wave-instructions of kernel `kern` priced with its measured opcode mix
                base = kern.replace("void ", "").split("<")[0].split("(")[0].strip()  # exact name: blur_kernel is a suffix of pyr_resize_blur_kernel
                m = next((v for kk, v in mix.items() if kk.split("<")[0] == base), None)
                return n * (m["mean_cycles_per_valu"] if m else ops["v_pk_max_i16"]["8"]["cycles_per_wave_inst_per_simd"]) / simd_cycles_per_s
            mf = next(v for k, v in mix.items() if "fast_cell_kernel" in k)
            out["frac_mix"] = seconds(insts, "fast_cell_kernel") / (launch_ms * 1e-3)
            out["mean_cycles_per_valu"] = mf["mean_cycles_per_valu"]
            out["full_rate_share"] = mf["full_rate_share"]
            out["mix_source"] = "profiles/" + os.path.basename(mix_path) + " (tools/isa_mix.py: opcode histogram of the disassembly per phase x measured cycles per opcode, phases weighted by SQ_INSTS_VALU)"
            whole["frac_mix"] = sum(seconds(n * pairs, k) for k, n in per_pair.items()) / (step_ms * 1e-3)
        out["whole_step"] = whole
        out["source"] = "replayed"
        return out
    except Exception:
        pass
    return None


def host_fed(api, torch, dev, host, P, make_ctx, steps=48, lanes_n=4):
    """PCIe-inclusive rate (never `value`): every step's P pairs start in PINNED host memory and the results end there.
    serial = upload -> chain -> download on one stream; overlapped = `lanes_n` lanes (fresh contexts, one stream each, step k on lane
    k % lanes_n), so one lane's copies run beside the others' kernels.  On this link the two directions at once take the SUM of their
    times (tools/pcie_rate.py, profiles/r03_pcie.json: 56 GB/s up alone, 55 GB/s down alone), so the bytes bound the rate.  Round 4:
    the results come down as ONE packed block (orbfe_fetch_batch_packed: 9 instead of 28 bytes per keypoint, uRight / depth of the
    left images only; expanded on the host by orbfe_expand_packed, bit-identical) and level 0 is read in place from the upload
    buffer (no ingest launch).  The block is written by the gather kernel straight into the pinned host block (ORBFE_PACK_DIRECT: posted
    writes across the link, no copy engine), which runs beside the uploads; the uploads of the lanes then keep the link busy
    (tools/r04_pcie_trace.sh: ~54 GB/s in steady state), so the rate approaches the upload-only bound of ~60 k pairs/s.  A pass is 48 steps
    (round 3: 16): pipeline fill and drain (one upload before the first kernel, one chain + download after the last upload, ~2 ms) are
    inside the timed region and cost a 16-step pass 12 %.  `unpacked` keeps round 3's five copies for comparison; `left_only` drops the
    right images' keypoints and descriptors as well (nothing outside ComputeStereoMatches reads them)."""
    h_in = torch.from_numpy(host).pin_memory()

    class Lane:
        def __init__(self, mode):
            self.ctx = make_ctx()
            self.stream = torch.cuda.Stream()
            self.d_in = torch.empty(h_in.shape, dtype=torch.uint8, device=dev)
            cap = self.ctx.capacity
            self.mode = mode
            if mode == "unpacked":
                self.sizes = [2 * P * cap * 28, 2 * P * cap * 32, 2 * P * 4, 2 * P * cap * 4, 2 * P * cap * 4]
                self.h_out = [torch.empty(n, dtype=torch.uint8).pin_memory() for n in self.sizes]
            else:
                self.flags = api.PACK_STEREO | api.PACK_DIRECT | (api.PACK_LEFT_ONLY if mode == "left_only" else 0)
                self.lay = self.ctx.packed_layout(2 * P, self.flags)
                self.sizes = [int(self.lay.bytes)]
                self.h_out = [torch.empty(self.lay.bytes, dtype=torch.uint8).pin_memory()]

        def step(self):
            with torch.cuda.stream(self.stream):
                self.d_in.copy_(h_in, non_blocking=True)
                self.ctx.enqueue_stereo(self.d_in.data_ptr(), P, self.stream.cuda_stream)
                if self.mode == "unpacked":
                    self.ctx.fetch_batch_async(2 * P, *[h.data_ptr() for h in self.h_out], self.stream.cuda_stream)
                else:
                    self.ctx.fetch_batch_packed(2 * P, self.flags, self.h_out[0].data_ptr(), self.sizes[0], self.stream.cuda_stream)

    def run(lanes):
        vals = []
        for rep in range(3):  # three short passes: one page-fault or clock stall otherwise decides a 16-step figure
            for l in lanes:
                l.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                lanes[k % len(lanes)].step()
            torch.cuda.synchronize()
            vals.append(P * steps / (time.perf_counter() - t0))
        return sorted(vals)[1], max(vals)

    out = {"unit": "frames/s", "lanes": lanes_n, "bytes_up_per_step": int(h_in.numel())}
    for mode in ("packed", "unpacked", "left_only"):
        lanes = [Lane(mode) for _ in range(lanes_n)]
        serial, _ = run(lanes[:1]) if mode == "packed" else (None, None)
        over, over_best = run(lanes)
        down = int(sum(lanes[0].sizes))
        if mode == "packed":  # the packed block of pair 0 expands to what the unpacked fetch of the same context delivers
            l0 = lanes[0]
            blk = l0.h_out[0].numpy()
            a, b = l0.ctx.expand_packed(blk, l0.lay, 0), l0.ctx.fetch_image(0, stereo=True)
            same = bool(a["kps"].tobytes() == b["kps"].tobytes() and np.array_equal(a["desc"], b["desc"]) and a["u_right"].tobytes() == b["u_right"].tobytes()
                        and a["depth"].tobytes() == b["depth"].tobytes())
            out.update({"serial": serial, "overlapped": over, "overlapped_best_of_3": over_best, "bytes_down_per_step": down, "packed_equals_unpacked": same})
        else:
            out[mode] = {"overlapped": over, "bytes_down_per_step": down}
        for l in lanes:
            l.ctx.close()
    up, dn = out["bytes_up_per_step"], out["bytes_down_per_step"]
    out["copy_bound"] = {"upload_only": P / (up / 56.1e9), "sum_of_both_directions": P / (up / 56.1e9 + dn / 54.8e9),
                         "note": "pairs/s at the rates measured alone (56.1 GB/s up, 54.8 GB/s down, profiles/r03_pcie.json): the upload alone, and a step's upload + download taking the sum of their times (what two copy-engine transfers in opposite directions do on this link)"}
    out["note"] = ("pinned host memory in and out; serial = one stream; overlapped = %d lanes (fresh contexts, one stream each); median of 3 passes of %d steps; "
                   "overlapped / bytes_down_per_step are the PACKED block written by the gather kernel into pinned host memory (round 4), `unpacked` = round 3's five "
                   "copies, `left_only` = without the right images' keypoints and descriptors" % (lanes_n, steps))
    return out


def small_batch(api, torch, d_images, P8, make_ctx, chains=4, steps=200, repeats=5):
    """BASELINE.json config 4 as worded -- 64 pairs in flight over 8 GPUs = 8 pairs per GPU per step: one chain of 15 dependent
    launches over 8 pairs is latency-bound, so `chains` step chains are kept in flight (step k on context k % chains)."""
    ctxs = [make_ctx(P8) for _ in range(chains)]
    streams = [torch.cuda.Stream() for _ in range(chains)]
    ptr = d_images.data_ptr()

    def run(n, c):
        for k in range(n):
            ctxs[k % c].enqueue_stereo(ptr, P8, streams[k % c].cuda_stream)

    def rate(c):
        run(4 * c, c)
        torch.cuda.synchronize()
        vals = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            run(steps, c)
            torch.cuda.synchronize()
            vals.append(P8 * steps / (time.perf_counter() - t0))
        return sorted(vals)
    v = rate(chains)
    v1 = rate(1)
    for c in ctxs:
        c.close()
    return {"pairs": P8, "chains_in_flight": chains, "value": v[len(v) // 2], "min": v[0], "max": v[-1], "ms_per_step": P8 / v[len(v) // 2] * 1e3,
            "one_chain_at_a_time": v1[len(v1) // 2], "steps": steps, "repeat": repeats, "unit": "frames/s"}


def natural_scene(api, torch, dev, P, make_ctx, steps=20):
    """The same step on a PHOTOGRAPH at the benchmark geometry (tests/natural.py: china.png enlarged to 1241 x 376 with the oracle's
    resize, right image = a crop 21 px apart with its own gain, offset and noise), one chain at a time: the generator's images have
    FAST corners on 16 % of all pixels, a real frame has large flat regions.  Checked against the oracle like the headline."""
    try:
        from tests import natural as N
        from oracle import oracle as O
        left, right, d, nf = N.pair("china_kitti")
    except Exception as e:  # the fixtures travel with the repository; a missing PIL is the only way here
        return {"error": str(e)}
    host = np.empty((2 * P, H, W), np.uint8)
    host[0::2], host[1::2] = left, right
    dimg = torch.from_numpy(host).to(dev)
    fx, fy, cx, cy, bf = N.camera(W, H)
    ctx = api.Context(width=W, height=H, nfeatures=nf, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, max_images=2 * P)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        ctx.enqueue_stereo(dimg.data_ptr(), P, st)
    torch.cuda.synchronize()
    vals = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.enqueue_stereo(dimg.data_ptr(), P, st)
        torch.cuda.synchronize()
        vals.append(P * steps / (time.perf_counter() - t0))
    ncand = sum(len(ctx.fetch_candidates(0, l)[0]) for l in range(NLEVELS))
    got = ctx.fetch_image(0, stereo=True)
    exl, exr = O.Extractor(nfeatures=nf), O.Extractor(nfeatures=nf)
    kl, dl = exl.extract(left); kr, dr = exr.extract(right)
    ur, dp, m = O.stereo_matches(exl, exr, kl, dl, kr, dr, bf, fx)
    ok = bool(len(got["kps"]) == len(kl) and np.array_equal(got["desc"], dl) and np.array_equal(got["u_right"], ur) and np.array_equal(got["kps"]["angle"], kl["angle"]))
    ctx.close()
    v = sorted(vals)[len(vals) // 2]
    return {"image": "china_kitti (photograph at 1241x376, tests/natural.py), %d copies per step" % P, "value": v, "ms_per_step": P / v * 1e3, "unit": "frames/s, one chain at a time",
            "fast_nms_candidates_per_image": ncand, "keypoints": int(len(kl)), "stereo_matches": int(m), "equals_oracle": ok}


def _median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def secondary_configs(api, torch, dev):
    """BASELINE.json configs 1, 3, 5 and the reference's own calling pattern (one Frame per call), untimed extras of the N = 1 line
    (round-3 verdict item 6): per-frame time through the HOST entry points (host buffers in and out, copies included), each checked
    against the oracle once.  tools/bench_configs.py is the long version (full-size vocabulary, CPU times)."""
    import ctypes as C
    from oracle import oracle as O
    from orbslam2_amd import bow as B, synth
    from tests import test_bow as TB
    out = {"unit": "ms per frame, median, host buffers in and out"}
    # config 1: Mono-TUM1 640x480 / 1000 features: ORBextractor::operator()
    W1, H1, N1 = 640, 480, 1000
    ctx = api.Context(width=W1, height=H1, nfeatures=N1, fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0, max_images=1)
    img = synth.mono_image(W1, H1, seed=5)
    k, d = ctx.extract(img)
    ko, do = O.Extractor(nfeatures=N1).extract(img)
    out["tum1_extract_ms"] = {"value": _median_ms(lambda: ctx.extract(img), 40), "equals_oracle": bool(np.array_equal(k, ko.astype(api.KP_DTYPE)) and np.array_equal(d, do)),
                              "config": "Mono-TUM1 640x480, 1000 features: orbfe_extract"}
    ctx.close()
    # config 3: Mono-EuRoC 752x480 / 1200 features: extract + fbow transform + 500-keyframe database query + SearchByFboW
    W3, H3, N3, NKF = 752, 480, 1200, 500
    ctx = api.Context(width=W3, height=H3, nfeatures=N3, fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=47.9, max_images=1)
    ex = O.Extractor(nfeatures=N3)
    base = [synth.mono_image(W3, H3, seed=900 + i) for i in range(20)]
    rng = np.random.default_rng(11)
    kf_kd = []
    for i in range(NKF):  # 500 keyframes: 20 scenes x 25 noise realisations (each its own keypoints / descriptors / BoW vector)
        im = base[i % 20]
        if i >= 20:
            im = np.clip(im.astype(np.int16) + rng.integers(-3, 4, im.shape, dtype=np.int16), 0, 255).astype(np.uint8)
        kf_kd.append(ctx.extract(im))
    blob = B.build_vocabulary(np.concatenate([dd for _, dd in kf_kd[:8]]), k=10, levels=4, seed=3)
    B.vocab_load(ctx, blob)
    L, v = TB._oracle_voc(blob)
    L.orc_detect_reloc_candidates.restype = C.c_int
    L.orc_detect_reloc_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int]
    db = B.KeyFrameDB(ctx)
    kf_bow, kf_fv = [], []
    for _, dd in kf_kd:
        w, wt, nd = B.transform(ctx, dd, 4)
        words, ww, nodes, off, feat = B.maps(w, wt, nd)
        db.add(words, ww)
        kf_bow.append((words, ww)); kf_fv.append((nodes, off, feat))
    q_img = np.clip(base[5].astype(np.int16) + rng.normal(0, 2.0, base[5].shape).round().astype(np.int16), 0, 255).astype(np.uint8)
    covis_off = np.arange(NKF + 1, dtype=np.int32) * 2
    covis_idx = np.stack([(np.arange(NKF) + 1) % NKF, (np.arange(NKF) - 1) % NKF], axis=1).astype(np.int32).ravel()
    kf_off = np.zeros(NKF + 1, np.int32); kf_off[1:] = np.cumsum([len(a) for a, _ in kf_bow])
    dbw = np.concatenate([a for a, _ in kf_bow]); dbv = np.concatenate([b for _, b in kf_bow])
    res = {}

    def gpu_chain():
        qk, qd = ctx.extract(q_img)
        gw, gwt, gnd = B.transform(ctx, qd, 4)
        q_words, q_ww, qn, qo, qf = B.maps(gw, gwt, gnd)
        st = np.zeros(NKF, np.float32)
        cand = db.detect_reloc_candidates(q_words, q_ww, covis_off, covis_idx, st)
        kfi = int(cand[0])
        kfk, kfd = kf_kd[kfi]
        m, nm = B.search_by_bow(ctx, kf_fv[kfi], np.ones(len(kfd), np.int32), kfd, kfk["angle"].copy(), (qn, qo, qf), qd, qk["angle"].copy(), 0.75, True)
        res["gpu"] = (cand.tolist(), nm)

    def cpu_chain():
        qk, qd = ex.extract(q_img)
        (w, wt, nd), (q_words, q_ww), q_fv = TB._oracle_transform(L, v, qd)
        st = np.zeros(NKF, np.float32); cand = np.zeros(NKF, np.int32)
        n = L.orc_detect_reloc_candidates(TB._p(q_words), TB._p(q_ww), len(q_words), NKF, TB._p(kf_off), TB._p(dbw), TB._p(dbv),
                                          TB._p(covis_off), TB._p(covis_idx), TB._p(st), TB._p(cand), NKF)
        kfi = int(cand[0])
        kfk, kfd = kf_kd[kfi]
        fv = kf_fv[kfi]
        ref = np.zeros(len(qd), np.int32)
        nref = L.orc_search_by_bow(TB._p(fv[0]), TB._p(fv[1]), TB._p(fv[2]), len(fv[0]), TB._p(np.ones(len(kfd), np.int32)), TB._p(kfd),
                                   TB._p(kfk["angle"].copy()), TB._p(q_fv[0]), TB._p(q_fv[1]), TB._p(q_fv[2]), len(q_fv[0]), TB._p(qd),
                                   TB._p(qk["angle"].copy()), len(qd), 0.75, 1, TB._p(ref))
        res["cpu"] = (cand[:n].tolist(), nref)

    g3 = _median_ms(gpu_chain, 25)
    cpu_chain()
    out["euroc_bow_reloc_ms"] = {"value": g3, "equals_oracle": bool(res["gpu"] == res["cpu"]), "matches": int(res["gpu"][1]), "keyframes": NKF,
                                 "config": "Mono-EuRoC 752x480, 1200 features: extract + fbow transform + 500-keyframe database query + SearchByFboW (k=10 / L=4 vocabulary trained on these images)"}
    L.orc_vocab_destroy(v)
    ctx.close()
    # config 5: D435i RGB-D 1280x720 / 2500 features: extract + ComputeStereoFromRGBD + SearchByProjection(last frame), per frame and batched
    W5, H5, N5 = 1280, 720, 2500
    fx = fy = 911.0; cx, cy, bf = 640.0, 360.0, 45.5
    ctx = api.Context(width=W5, height=H5, nfeatures=N5, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, max_images=1)
    ex = O.Extractor(nfeatures=N5)
    img1, img2, depth = synth.stereo_pair(W5, H5, seed=321, with_depth=True, bf=bf)
    f1 = ctx.rgbd_frame(img1, depth)
    z = f1["depth"]
    valid = (z > 0).astype(np.int32)
    pos = np.stack([(f1["kps"]["x"] - cx) * z / fx, (f1["kps"]["y"] - cy) * z / fy, z], axis=1).astype(np.float32)
    obs = np.ones(len(z), np.int32)
    T_last = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    T_cur = T_last.copy(); T_cur[0, 3] = -bf / fx
    bounds = (0.0, float(W5), 0.0, float(H5))
    cam = O.Camera(fx, fy, cx, cy, bf, bf / fx)
    k1o, d1o = ex.extract(img1)
    r5 = {}

    def gpu5():
        f2 = ctx.rgbd_frame(img2, depth)
        view = ctx._view(f2["kps"], f2["u_right"], f2["desc"], bounds, device_slot=0)  # the frame just extracted, matched where it lies in HBM
        got, n = ctx.search_by_projection_last(view, T_cur, T_last, pos, f1["desc"], valid, obs, f1["kps"]["octave"].copy(),
                                               f1["kps"]["angle"].copy(), None, 7.0, False, True)
        r5["g"] = (n, got)

    g5 = _median_ms(gpu5, 25)
    k2, d2 = ex.extract(img2)
    ur2, dp2 = O.stereo_from_rgbd(k2, k2, depth, bf)
    ref, nref = O.search_by_projection_last(O.Grid(k2, *bounds), ur2, d2, ex.scale_factors(), cam, T_cur, T_last, pos, d1o, valid, obs,
                                            k1o["octave"].copy(), k1o["angle"].copy(), None, 7.0, False, True)
    out["d435i_rgbd_track_ms"] = {"value": g5, "equals_oracle": bool(r5["g"][0] == nref and np.array_equal(r5["g"][1], ref)), "matches": int(nref),
                                  "config": "RealSense-D435i RGB-D 1280x720, 2500 features: orbfe_rgbd_frame + SearchByProjection(last frame) on the resident frame"}
    ctx.close()
    # the same configuration batched: 32 frames per step through orbfe_enqueue_rgbd (grey + float depth resident in HBM), one chain at a time
    NB = 32
    ctx = api.Context(width=W5, height=H5, nfeatures=N5, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, max_images=NB)
    gray = np.empty((NB, H5, W5), np.uint8); dep = np.empty((NB, H5, W5), np.float32)
    gray[0::2], gray[1::2] = img1, img2
    dep[:] = depth
    d_gray, d_dep = torch.from_numpy(gray).to(dev), torch.from_numpy(dep).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        ctx.enqueue_rgbd(d_gray.data_ptr(), d_dep.data_ptr(), NB, stream=st)
    torch.cuda.synchronize()
    vals = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            ctx.enqueue_rgbd(d_gray.data_ptr(), d_dep.data_ptr(), NB, stream=st)
        torch.cuda.synchronize()
        vals.append(NB * 10 / (time.perf_counter() - t0))
    got = ctx.fetch_image(1, stereo=True)
    okb = bool(got["kps"].tobytes() == k2.astype(api.KP_DTYPE).tobytes() and np.array_equal(got["desc"], d2) and np.array_equal(got["u_right"], ur2) and np.array_equal(got["depth"], dp2))
    v5 = sorted(vals)[len(vals) // 2]
    out["d435i_rgbd_batched"] = {"value": v5, "unit": "frames/s", "frames_per_step": NB, "ms_per_step": NB / v5 * 1e3, "equals_oracle": okb,
                                 "config": "the same camera, 32 frames per step resident in HBM: orbfe_enqueue_rgbd (extract + ComputeStereoFromRGBD in one chain), one chain at a time"}
    ctx.close()
    return out


def single_frame(api, torch, dev):
    """The reference's own calling pattern -- ONE Frame per call (src/Tracking.cc:296: Frame(left, right, ...)): the stereo frame of
    the headline configuration through orbfe_stereo_frame (host images in, host keypoints / descriptors / uRight / depth out), and
    with the pair already in HBM and the results left there."""
    from orbslam2_amd import synth
    left, right = synth.stereo_pair(W, H, seed=1234)
    ctx = api.Context(width=W, height=H, nfeatures=NFEAT, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF, max_images=2)
    h2h = _median_ms(lambda: ctx.stereo_frame(left, right), 50, 5)
    d = torch.from_numpy(np.stack([left, right])).to(dev)
    torch.cuda.synchronize()

    def resident():
        ctx.enqueue_stereo(d.data_ptr(), 1)
        ctx.synchronize()
    res = _median_ms(resident, 50, 5)
    ctx.close()
    return {"stereo_host_to_host_ms": h2h, "stereo_resident_ms": res, "unit": "ms per frame pair, median of 50",
            "note": "orbfe_stereo_frame (pageable host images in, host results out) / orbfe_enqueue_stereo + synchronise on a pair resident in HBM"}


def cpu_baseline(n_pairs: int):
    """Oracle (kind=port) timed with the reference's threading: 2 threads per pair (src/Frame.cc:78-81)."""
    from oracle import oracle as O
    from orbslam2_amd import synth
    target = "liborb_oracle_fast.so"
    pairs = [synth.stereo_pair(W, H, seed=5000 + i) for i in range(min(n_pairs, 4))]
    exl = O.Extractor(nfeatures=NFEAT, target=target)
    exr = O.Extractor(nfeatures=NFEAT, target=target)

    def one(pair):
        res = [None, None]
        def run(i, ex, img):
            res[i] = ex.extract(img)
        tl = threading.Thread(target=run, args=(0, exl, pair[0]))
        tr = threading.Thread(target=run, args=(1, exr, pair[1]))
        tl.start(); tr.start(); tl.join(); tr.join()
        (kl, dl), (kr, dr) = res
        O.stereo_matches(exl, exr, kl, dl, kr, dr, BF, FX)

    one(pairs[0])  # warm-up
    t0 = time.perf_counter()
    for i in range(n_pairs):
        one(pairs[i % len(pairs)])
    dt = time.perf_counter() - t0
    out = {"value": n_pairs / dt, "unit": "frames/s", "cores": 2, "kind": "port",
           "sample": "%d KITTI-geometry synthetic stereo pairs, oracle -O3 -march=native, 2 threads/pair "
                     "(reference threading), %.1f s" % (n_pairs, dt)}
    # every host core busy -- floor(cores / 2) pairs at a time, each with the reference's 2 threads
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 2)
    workers = max(1, min(ncpu // 2, 8))  # the GPU box grants one GPU's share of the host: 16 cores
    if workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        exs = [(O.Extractor(nfeatures=NFEAT, target=target), O.Extractor(nfeatures=NFEAT, target=target)) for _ in range(workers)]

        def worker(wi, count):
            el, er = exs[wi]
            for k in range(count):
                pl, pr = pairs[(wi + k) % len(pairs)]
                res = [None, None]
                def run(i, ex, img):
                    res[i] = ex.extract(img)
                tl = threading.Thread(target=run, args=(0, el, pl)); tr = threading.Thread(target=run, args=(1, er, pr))
                tl.start(); tr.start(); tl.join(); tr.join()
                O.stereo_matches(el, er, res[0][0], res[0][1], res[1][0], res[1][1], BF, FX)

        per = max(4, n_pairs // (3 * workers))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(lambda wi: worker(wi, per), range(workers)))
        dt2 = time.perf_counter() - t0
        out["all_cores"] = {"value": workers * per / dt2, "cores": 2 * workers,
                            "sample": "%d pairs, %d at a time x 2 threads, %.1f s" % (workers * per, workers, dt2)}
    return out


def strong_pass(args, D, torch, make_ctx, d_images, share, P_total, world, cdev):
    """BASELINE config 4 as worded on N ranks: P_total pairs per step in total, `share` of them on this rank (the first `share`
    pairs of its resident batch), timed with the headline protocol (barrier + synchronize around EXACTLY --steps steps, MAX over
    ranks, median of 3) with 1 and with --strong-chains step chains in flight.  Every step is enqueued exactly once, on context
    k % chains (dist.chain_schedule); every rank runs all steps of its own share, so a step covers every pair exactly once."""
    SC = max(1, min(args.strong_chains, 8))
    ctxs = [make_ctx(share) for _ in range(SC)]
    streams = [torch.cuda.Stream() for _ in range(SC)]
    ptr = d_images.data_ptr()

    def run(chains):
        for k, c in D.chain_schedule(args.steps, chains):
            ctxs[c].enqueue_stereo(ptr, share, streams[c].cuda_stream)

    def timed(chains):
        D.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(chains)
        D.barrier(); torch.cuda.synchronize()
        return D.max_over_ranks(time.perf_counter() - t0, cdev)

    out = {"pairs_per_step_total": P_total, "pairs_per_step_per_gpu": [len(D.shard_pairs(P_total, r, world)) for r in range(world)]}
    for chains in sorted({1, SC}):
        run(chains)  # warm-up: every context once
        dt = sorted(timed(chains) for _ in range(3))[1]
        out["one_chain" if chains == 1 else "chains_%d" % chains] = {"chains_in_flight": chains, "value": P_total * args.steps / dt, "ms_per_step": dt / args.steps * 1e3}
    best = out.get("chains_%d" % SC, out["one_chain"])
    out.update({"value": best["value"], "ms_per_step": best["ms_per_step"], "chains_in_flight": best["chains_in_flight"],
                "note": "same timing protocol (median of 3); `value` = the %d-chain figure (the product mode for small per-GPU batches), one_chain beside it" % best["chains_in_flight"]})
    for c in ctxs:
        c.close()
    return out


DUMP_BUDGET = 64 << 20  # --dump-outputs: bytes of .npy data at most
WARM_S = 0.25  # without --full: warm-up steps go on until the chip has been busy this long (at least --warmup steps)


def dump_outputs(ctx, n_pairs, out_dir, budget=DUMP_BUDGET):
    """--dump-outputs DIR: what a caller of the timed path receives from its last step, as float32 .npy files, so that two builds
    can be compared output for output.  Per stereo pair: the left and the right keypoints (cv::KeyPoint fields x, y, size, angle,
    response, octave, class_id), their descriptors (32 bytes, one column each) and uRight / depth of the left keypoints; the images
    of the dumped pairs are concatenated in pair order and counts_left / counts_right say how many keypoints each one holds.  All
    pairs while the worst case (every image at keypoint capacity) fits in `budget` bytes, else a fixed seeded sample of pairs;
    pairs.npy lists the pairs dumped.  Written by rank 0 from its own batch."""
    per_pair = ctx.capacity * (2 * (7 + 32) * 4 + 2 * 4) + 3 * 4
    k = max(1, min(n_pairs, budget // per_pair))
    pairs = np.arange(n_pairs) if k == n_pairs else np.sort(np.random.default_rng(0).choice(n_pairs, k, replace=False))
    cols = ("x", "y", "size", "angle", "response", "octave", "class_id")
    got = {"left": [], "right": []}
    for i in pairs:
        got["left"].append(ctx.fetch_image(2 * int(i), stereo=True))
        got["right"].append(ctx.fetch_image(2 * int(i) + 1))
    arrays = {"pairs": pairs.astype(np.float32)}
    for side, imgs in got.items():
        kps = np.concatenate([g["kps"] for g in imgs])
        arrays["counts_" + side] = np.array([len(g["kps"]) for g in imgs], np.float32)
        arrays["keypoints_" + side] = np.stack([kps[c].astype(np.float32) for c in cols], 1)
        arrays["descriptors_" + side] = np.concatenate([g["desc"] for g in imgs]).astype(np.float32)
    arrays["u_right"] = np.concatenate([g["u_right"] for g in got["left"]]).astype(np.float32)
    arrays["depth"] = np.concatenate([g["depth"] for g in got["left"]]).astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher environment (the way the driver starts the N = 1 run): this process starts
    the N ranks itself -- one child per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, exactly what torch.distributed.run
    would export -- BEFORE anything here touches the GPU (it never does: no torch import, no HIP call), relays rank 0's one JSON
    line and returns non-zero unless every rank exits 0 and the line says n_gpus == N.  A rank that dies takes the others with it
    (they would otherwise wait in the rendezvous)."""
    import socket
    import subprocess
    # The rendezvous port is found by binding to port 0 and closing the socket: another process can take it before rank 0 listens
    # there (rank 0 then dies with "address already in use").  That, and only that, is retried with a fresh port.
    for attempt in range(3):
        rc = _launch_once(n, socket, subprocess)
        if rc != "port-taken":
            return rc
        print("bench: rendezvous port was taken before rank 0 could bind it; retrying with another (%d)" % (attempt + 1), file=sys.stderr)
    return 1


def _launch_once(n, socket, subprocess):
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   ORBFE_BENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=subprocess.PIPE if r == 0 else sys.stderr))
    line = {"err": b""}

    def read0():
        line["out"] = procs[0].stdout.read()

    def tee0():  # rank 0's stderr goes through to ours, and its tail is kept: the one message the launcher reacts to is a bind failure
        for chunk in iter(lambda: procs[0].stderr.read1(4096), b""):
            sys.stderr.buffer.write(chunk); sys.stderr.flush()
            line["err"] = (line["err"] + chunk)[-8192:]
    t = threading.Thread(target=read0, daemon=True)
    t.start()
    t2 = threading.Thread(target=tee0, daemon=True)
    t2.start()
    rcs = [None] * n
    failed = None
    deadline = time.time() + float(os.environ.get("ORBFE_BENCH_LAUNCH_TIMEOUT_S", "3000"))  # a rank that hangs must not hang the launcher for ever
    while any(rc is None for rc in rcs):
        if time.time() > deadline:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            for p in procs:  # reap them, and let the reader threads see end-of-file before their output is dropped
                try:
                    p.wait(15)
                except subprocess.TimeoutExpired:
                    pass
            t.join(15); t2.join(15)
            print("bench: the %d-rank run did not finish within ORBFE_BENCH_LAUNCH_TIMEOUT_S; killed" % n, file=sys.stderr)
            return 1
        for r, p in enumerate(procs):
            if rcs[r] is None:
                rcs[r] = p.poll()
                if rcs[r] not in (None, 0) and failed is None:
                    failed = r
        if failed is not None:
            break
        time.sleep(0.05)
    if failed is not None:
        for r, p in enumerate(procs):
            if p.poll() is None:
                p.terminate()  # our own children, by handle
        for p in procs:
            try:
                p.wait(15)
            except subprocess.TimeoutExpired:
                p.kill()
        t.join(15); t2.join(15)
        err = line["err"].decode("utf-8", "replace").lower()
        if failed == 0 and ("address already in use" in err or "eaddrinuse" in err):
            return "port-taken"
        print("bench: rank %d exited with code %d; %d-rank run aborted" % (failed, rcs[failed], n), file=sys.stderr)
        return rcs[failed] if 0 < rcs[failed] < 256 else 1
    t.join(30); t2.join(30)
    text = (line.get("out") or b"").decode("utf-8", "replace")
    rows = [ln for ln in text.splitlines() if ln.strip().startswith("{")]
    if len(rows) != 1:
        print("bench: expected ONE JSON line from rank 0, got %d" % len(rows), file=sys.stderr)
        return 1
    try:
        got = json.loads(rows[0]).get("n_gpus")
    except Exception as e:
        print("bench: rank 0's line is not JSON (%s)" % e, file=sys.stderr)
        return 1
    if got != n:
        print("bench: rank 0 reports n_gpus %r, --gpus %d" % (got, n), file=sys.stderr)
        return 1
    print(rows[0], flush=True)
    return 0


def launcher_selftest(args, D, rank, world, real_stdout):
    """--launcher-selftest: the distributed plumbing of the N > 1 run and nothing else, over gloo on CPU tensors (tests/test_bench_launcher.py):
    rendezvous, rank count, parameter + pattern-checksum broadcast, vocabulary broadcast, MAX all-reduce, one line from rank 0."""
    import torch
    import torch.distributed as dist
    cdev = torch.device("cpu")
    D.init("gloo", None, force=True)
    joined = D.count_ranks(cdev)
    if joined != world:
        raise SystemExit("bench: %d ranks joined the process group, --gpus %d" % (joined, args.gpus))
    params_blob = D.pack_params(NFEAT, 1.2, NLEVELS, 20, 7, 31, 15, 19, FX, FY, CX, CY, BF)
    blob = D.broadcast_params(params_blob if rank == 0 else D.pack_params(1, 2.0, 3, 40, 30, 31, 15, 19, 1.0, 1.0, 0.0, 0.0, 1.0), cdev)
    assert D.unpack_params(blob)[0] == NFEAT
    voc = D.broadcast_blob(bytes(range(256)) * 16 if rank == 0 else None, cdev)
    t = D.max_over_ranks(1.0 + rank, cdev)
    assert t == float(world), t
    # the strong-scaling pass with chains in flight (strong_pass): every (step, pair) is enqueued exactly once over all ranks and chains
    pat = D.broadcast_pattern(D.compiled_pattern() if rank == 0 else None, cdev)
    assert pat.shape == (256, 4)
    SC = max(1, min(args.strong_chains, 8))
    mine = D.shard_pairs(args.pairs, rank, world)
    cover = [(k, c, p) for k, c in D.chain_schedule(args.steps, SC) for p in mine]
    allc = [None] * world
    dist.all_gather_object(allc, cover)
    seen = {}
    for r, cv in enumerate(allc):
        for k, c, p in cv:
            seen.setdefault((k, p), []).append((r, c))
    strong_ok = (sorted(seen) == [(k, p) for k in range(args.steps) for p in range(args.pairs)] and all(len(v) == 1 for v in seen.values())
                 and all(c == k % SC for cv in allc for k, c, _ in cv))
    D.barrier()
    if rank == 0:
        out = {"selftest": "launcher", "n_gpus": joined, "value": None, "strong_cover_exactly_once": bool(strong_ok), "strong_chains": SC,
               "config": {"rccl": {"ranks": joined, "backend": "gloo", "broadcast_bytes": len(params_blob) + len(voc) + 8 + 32,
                                   "self_launched": os.environ.get("ORBFE_BENCH_SELF_LAUNCHED") == "1"}}}
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    D.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=64, help="stereo pairs per step per GPU (in flight in HBM; BASELINE.json config 4 batches 64 pairs)")
    ap.add_argument("--chains", type=int, default=0, help="0 = 1 in --mode weak, --strong-chains in --mode strong; step chains in flight per GPU in the HEADLINE region: step k runs on context k %% chains and its stream (1 = one chain at a time)")
    ap.add_argument("--full", action="store_true", help="besides the headline, everything else the benchmark measures and checks: the repeated timed region, "
                    "the roofline and per-stage table, the pipelined / one-chain / strong-scaling passes, small batch, natural image, secondary configs, "
                    "host-fed rate, CPU baseline and the oracle spot check.  Without it a run sets up, warms up, times exactly --steps steps once and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32; dump_outputs)")
    ap.add_argument("--pipelined", type=int, default=3, help="--full: after the headline region, time the same steps with this many chains in flight -> config.pipelined (0 / 1 = skip)")
    ap.add_argument("--repeat", type=int, default=None, help="the timed region (--steps steps) is repeated this often; value = median, config.repeat = min / max (default 5 with --full, else 1)")
    ap.add_argument("--min-region-ms", type=float, default=None, help="keep repeating the timed region until the regions add up to this much timed GPU work (at most 64 regions; default 100 with --full, else 0)")
    ap.add_argument("--strong-chains", type=int, default=4, help="step chains in flight in the strong-scaling regime (the strong pass beside a weak run: --full) (8 pairs per GPU per step at N = 8 are launch-latency-bound with one): --mode strong runs its headline with this many, the strong pass beside a weak run reports 1 and this many")
    ap.add_argument("--streams", type=int, default=1, help="stream groups the batch is cut into inside the library (1 keeps per-kernel times clean)")
    ap.add_argument("--cpu-pairs", type=int, default=300, help="--full: pairs in the CPU baseline sample (0 = skip)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (nccl = RCCL; gloo only for rehearsals)")
    ap.add_argument("--no-check", action="store_true", help="--full: skip the post-run oracle spot check")
    ap.add_argument("--mode", default="weak", choices=["weak", "strong"], help="weak: --pairs per GPU; strong: --pairs in total, sharded by dist.shard_pairs")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic pairs the batch cycles through")
    ap.add_argument("--host-fed", type=int, default=1, help="--full, 1: after the timed region also measure the PCIe-inclusive rate (N = 1 only; never `value`)")
    ap.add_argument("--rehearse-rccl", action="store_true", help="N = 1: run over a ONE-RANK process group of --backend, so a one-GPU box exercises the very RCCL calls of the multi-GPU path (parameter / vocabulary broadcast, barrier, MAX all-reduce)")
    ap.add_argument("--natural", type=int, default=1, help="--full, 1: N = 1 only, also time the step on a photograph at the benchmark geometry -> config.natural_image")
    ap.add_argument("--small-batch", type=int, default=8, help="--full, N = 1 only: also time steps of this many pairs (BASELINE config 4's 8 pairs per GPU) with 4 chains in flight -> config.small_batch; 0 = skip")
    ap.add_argument("--secondary", type=int, default=1, help="--full, 1: N = 1 only, also time BASELINE configs 1, 3, 5 and the one-Frame-per-call pattern through the host entry points -> config.secondary, config.single_frame")
    ap.add_argument("--launcher-selftest", action="store_true", help="CPU-only check of the N > 1 plumbing (self-launch, rendezvous, the one-time broadcasts, rank count, exit codes); prints the line's distributed fields and runs NO compute")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench: --gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("bench: --steps must be >= 1")
    if args.repeat is None:
        args.repeat = 5 if args.full else 1
    if args.min_region_ms is None:
        args.min_region_ms = 100.0 if args.full else 0.0

    # --gpus N > 1 without a launcher's environment: this process becomes the launcher.  It never touches the GPU.
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))

    # Rank 0 prints ONE JSON line on stdout and nothing else: RCCL writes its version banner ("RCCL version : ... Librccl path : ...")
    # to STDOUT when the first communicator is created, and other libraries may chat there too, so file descriptor 1 points at stderr
    # until the line is ready.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    from orbslam2_amd import dist as D
    rank, local_rank, world = D.world_info()
    # Never a silent fallback: a launcher that started a different number of ranks than --gpus asks for is an error on every rank
    # (round-3 verdict: `python3 bench.py --gpus 8` used to report a one-GPU result with n_gpus 1).
    if world != args.gpus:
        raise SystemExit("bench: --gpus %d but the launcher environment says WORLD_SIZE=%d (rank %d): refusing to report a %d-rank run as %d GPUs"
                         % (args.gpus, world, rank, world, args.gpus))
    if os.environ.get("ORBFE_BENCH_FAIL_RANK") == str(rank):  # test hook: a rank that dies before the rendezvous
        raise SystemExit(3)
    if args.launcher_selftest:
        return launcher_selftest(args, D, rank, world, real_stdout)

    import torch
    import torch.distributed as dist
    from orbslam2_amd import api, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    # --backend gloo with ORBFE_BENCH_ONE_GPU=1 rehearses the multi-rank path on a one-GPU box (all ranks on device 0,
    # collectives on CPU tensors); the real run is one rank per GPU over RCCL.
    one_gpu = args.backend == "gloo" and os.environ.get("ORBFE_BENCH_ONE_GPU") == "1"
    ndev = torch.cuda.device_count()
    # a launcher may give every rank its own single visible device (HIP_VISIBLE_DEVICES per rank): then the rank's GPU is index 0
    masked = not one_gpu and world > 1 and ndev == 1 and os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("CUDA_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))) is not None
    if not one_gpu and not masked and ndev < world:
        raise SystemExit("bench: %d ranks but only %d GPU(s) visible (one rank per GPU; ORBFE_BENCH_ONE_GPU=1 --backend gloo rehearses on one)"
                         % (world, ndev))
    gpu_index = 0 if (one_gpu or masked) else local_rank
    torch.cuda.set_device(gpu_index)
    dev = torch.device("cuda", gpu_index)
    cdev = dev if args.backend == "nccl" else torch.device("cpu")  # where the collectives' tensors live
    D.init(args.backend, dev, force=args.rehearse_rccl)
    ranks_joined = D.count_ranks(cdev)  # SUM all-reduce of 1 over the group: what RCCL itself saw
    if ranks_joined != world:
        raise SystemExit("bench: %d ranks joined the process group, --gpus %d" % (ranks_joined, args.gpus))

    # one-time RCCL broadcast of the extractor parameters + rBRIEF pattern checksum
    params_blob = D.pack_params(NFEAT, 1.2, NLEVELS, 20, 7, 31, 15, 19, FX, FY, CX, CY, BF)
    blob = D.broadcast_params(params_blob, cdev)
    nf, sf, nl, ini, mn, ps, hps, et, fx, fy, cx, cy, bf = D.unpack_params(blob)
    # ... and of the rBRIEF test table itself (north_star: "RCCL broadcast of the ORB pattern"): rank 0's 256 x 4 integers travel, every
    # rank hands them to its contexts (orbfe_set_pattern), as ORBextractor copies the table per object (src/ORBextractor.cc:442-444)
    pattern = D.broadcast_pattern(D.compiled_pattern() if rank == 0 else None, cdev)

    # one-time RCCL broadcast of the vocabulary (fbow file format) from rank 0 into every rank's HBM: the only other
    # xGMI traffic north_star allows.  Synthetic k = 10 / L = 3 tree here (no vocabulary file ships with the repo).
    voc_blob = None
    if world > 1 or args.rehearse_rccl:
        from orbslam2_amd import bow as BOW
        if rank == 0:
            rng = np.random.default_rng(99)
            voc_blob = BOW.build_vocabulary(rng.integers(0, 256, (4000, 32), dtype=np.uint8), k=10, levels=3)
        voc_blob = D.broadcast_blob(voc_blob, cdev)

    P_total = args.pairs
    mine = D.shard_pairs(P_total, rank, world)  # strong-scaling share of this rank
    P = args.pairs if args.mode == "weak" else len(mine)
    if P < 1:
        raise SystemExit("bench: --mode strong needs --pairs >= number of GPUs")
    if args.chains <= 0:
        args.chains = 1 if args.mode == "weak" else args.strong_chains
    C = max(1, min(args.chains, 8))
    CP = max(C, min(args.pipelined, 8)) if args.full and args.pipelined > 1 else C  # contexts needed in all
    G = max(1, min(args.streams, P, 8))

    def make_ctx(pairs=P):
        c = api.Context(width=W, height=H, nfeatures=nf, scale_factor=sf, nlevels=nl, ini_th_fast=ini, min_th_fast=mn,
                        patch_size=ps, half_patch_size=hps, edge_threshold=et, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                        device=gpu_index, max_images=2 * pairs)
        c.set_pattern(pattern)  # the broadcast table, not the compiled-in one (equal here; a deployment may distribute its own)
        return c

    ctxs = [make_ctx() for _ in range(CP)]
    for c in ctxs:
        c.set_streams(G)
    ctx = ctxs[0]
    if voc_blob is not None:
        BOW.vocab_load(ctx, voc_blob)
    host = np.empty((2 * P, H, W), np.uint8)
    if args.mode == "weak":  # every rank its own pairs
        n_distinct = max(1, min(P, args.distinct))
        distinct = [synth.stereo_pair(W, H, seed=1234 + rank * 100 + i) for i in range(n_distinct)]
        for i in range(P):
            host[2 * i], host[2 * i + 1] = distinct[i % n_distinct]
    else:  # one global list of P_total pairs, rank r extracts pairs r, r + world, ...
        n_distinct = max(1, min(P_total, args.distinct))
        cache = {}
        for j, gi in enumerate(mine):
            k = gi % n_distinct
            if k not in cache:
                cache[k] = synth.stereo_pair(W, H, seed=1234 + k)
            host[2 * j], host[2 * j + 1] = cache[k]
    d_images = torch.from_numpy(host).to(dev)
    # every chain on a stream of its own (kernels are launched there, and the library's HIP events are recorded there)
    streams = [torch.cuda.Stream(device=dev) for _ in range(CP)]
    n_step = [P]
    k_step = [0]

    def step(chains=C):
        i = k_step[0] % chains
        k_step[0] += 1
        ctxs[i].enqueue_stereo(d_images.data_ptr(), n_step[0], streams[i].cuda_stream)

    def barrier():
        D.barrier()
        torch.cuda.synchronize()  # the whole device: every chain's stream

    def timed(steps, chains=C):
        k_step[0] = 0
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(chains)
        barrier()
        return D.max_over_ranks(time.perf_counter() - t0, cdev)

    n_warm = max(args.warmup, CP)
    for _ in range(n_warm):  # every chain's context runs at least once before the clock starts
        step(CP)
    barrier()
    if not args.full:  # one timed region only: it starts on a chip that has been busy for a while (--full's first region of 5 does not)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < WARM_S:  # ranks may run different counts: local synchronise, one barrier after
            for _ in range(16):
                step(CP)
            torch.cuda.synchronize()
            n_warm += 16
        barrier()
    # Timed region (--full): HIP events only around the dominant kernel (cell-wise FAST, stage 3) on the stream of its chain -- an
    # event at every stage boundary costs ~6 us of idle GPU each, i.e. ~6 % of a step.  The full per-stage table comes from a
    # separate, untimed single-chain pass after the timed region.  Without --full the timed region records no events.
    DOM = "fast"
    EVERY = 10  # events on every 10th step of a chain (two recorded steps per 20-step repeat): the two events of a step cost ~2 % of it
    if args.full:
        for c in ctxs[:C]:
            c.set_profiling(2 + api.STAGE_NAMES.index(DOM))
            c.set_profiling_interval(EVERY)
    R = max(1, args.repeat)
    dts, dom_ms_sum, dom_calls = [], 0.0, 0
    # the region of EXACTLY --steps steps (barrier + synchronize on both sides) is repeated at least --repeat times and until the
    # regions add up to --min-region-ms of timed GPU work (--full: 5 times and 100 ms, as 20 steps are ~13 ms: too short for a
    # stable median on a fresh box; otherwise once); value = the median region, config.repeat = n / min / max
    while len(dts) < R or (sum(dts) * 1e3 < args.min_region_ms and len(dts) < 64):
        dts.append(timed(args.steps))
        if args.full:
            for c in ctxs[:C]:
                ms, calls = c.stage_times(reset=True)
                dom_ms_sum += ms[DOM]; dom_calls += calls
    R = len(dts)
    dt = sorted(dts)[len(dts) // 2]
    if args.dump_outputs and rank == 0:  # the last timed step ran on context (steps - 1) % C
        dump_outputs(ctxs[(args.steps - 1) % C], P, args.dump_outputs)
    dom_alone = single = piped = strong = None
    if args.full:
        # the dominant kernel alone on the chip (one chain at a time): what the co-scheduled figure of the timed region stretches
        for c in ctxs:
            c.set_profiling_interval(1)
        if C > 1:
            k_step[0] = 0
            for _ in range(min(args.steps, 10)):
                step(1)
            barrier()
            ms, calls = ctx.stage_times(reset=True)
            dom_alone = ms[DOM] / max(calls, 1) / G
        for c in ctxs:
            c.set_profiling(0)
        if C > 1:  # one chain at a time beside it, no events
            single = sorted(timed(args.steps, 1) for _ in range(3))[1]
        if CP > C:  # the deployment regime: CP step chains in flight, same steps, same barrier protocol, no events
            for _ in range(CP):
                step(CP)
            piped = sorted(timed(args.steps, CP) for _ in range(R))
        ctx.set_profiling(1)
        k_step[0] = 0
        for _ in range(min(args.steps, 10)):
            step(1)
        barrier()
        stage_ms, calls = ctx.stage_times(reset=True)
        for c in ctxs:
            c.set_profiling(0)

        # strong-scaling pass beside a weak run on several GPUs: P_total pairs in total, this rank's share per step -- with ONE step
        # chain and with --strong-chains chains in flight (contexts sized for the share, step k on context k % chains: the product mode
        # of config.small_batch; 8 pairs per GPU per step are launch-latency-bound with one chain, which says nothing about xGMI)
        if args.mode == "weak" and world > 1 and len(mine) >= 1:
            strong = strong_pass(args, D, torch, make_ctx, d_images, len(mine), P_total, world, cdev)
        k_step[0] = 0
        step(1)  # leave the full batch's results in context 0 for the checks below
        barrier()

    counts = ctx.fetch_counts(2 * P)
    n_cand = 0
    if rank == 0 and args.full:
        n_cand = sum(len(ctx.fetch_candidates(0, l)[0]) for l in range(nl))
        if not args.no_check:  # the timed path must be the correct path: spot-check pair 0 of EVERY chain's context against the oracle
            from oracle import oracle as O
            exl, exr = O.Extractor(nfeatures=nf), O.Extractor(nfeatures=nf)
            kl, dl = exl.extract(host[0]); kr, dr = exr.extract(host[1])
            ur, dp, _ = O.stereo_matches(exl, exr, kl, dl, kr, dr, bf, fx)
            for c in ctxs:
                got = c.fetch_image(0, stereo=True)
                ok = (len(got["kps"]) == len(kl) and np.array_equal(got["desc"], dl) and np.array_equal(got["u_right"], ur)
                      and np.array_equal(got["kps"]["x"], kl["x"]) and np.array_equal(got["kps"]["angle"], kl["angle"]))
                if not ok:
                    raise SystemExit("bench: HIP output differs from the oracle -- result invalid")

    if rank == 0:
        pairs_per_step = P * world if args.mode == "weak" else P_total
        value = pairs_per_step * args.steps / dt
        metric = "frames/sec ORB extract+match, KITTI 1241x376 stereo, 2000 feats"
        try:
            metric = json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
        except Exception:
            pass
        step_ms = dt / args.steps * 1e3
        roof = None
        if args.full:
            alg = stage_alg_bytes_per_pair(n_cand)
            # stage time per step, summed over the G stream groups (they overlap in wall time)
            per_launch_ms = {k: v / max(calls, 1) for k, v in stage_ms.items()}
            dom = DOM
            if max(per_launch_ms, key=per_launch_ms.get) != DOM:
                print("bench: note: stage %s is now longer than %s" % (max(per_launch_ms, key=per_launch_ms.get), DOM), file=sys.stderr)
            launches = G  # per step a stage is G launches (one per stream group)
            dom_ms = dom_ms_sum / max(dom_calls, 1) / launches  # from the events of the timed region, on the launching stream
            # FAST's launch also carries the blur of the levels the pyramid launches leave unblurred: level NLEVELS - 1 for batches of
            # 64 images and more per launch (smaller batches carry more levels: not counted, i.e. understated); its algorithmic bytes
            # (one read, one write of the level, SURVEY's blur row) belong to the launch that does the work
            riding = list(range(ctx.blur_ride_from(2 * P // launches), NLEVELS)) if dom == "fast" else []  # orbfe_blur_ride_from: the plan the library actually runs
            dom_alg = alg[dom] + sum(2 * 2 * LEVEL_PX[l] for l in riding)
            achieved = dom_alg * P / launches / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
            roof = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic_bytes(dom, P, launches),
                    "launch_ms": dom_ms, "alg_bytes_per_launch": dom_alg * P / launches, "blur_levels_riding_in_launch": riding,
                    "events_every_nth_step": EVERY,
                    "valu_issue": valu_issue(P, launches, dom_ms, step_ms),
                    "whole_pipeline": {"alg_bytes_per_pair": B_PAIR, "achieved": B_PAIR * value / world / 1e9,
                                       "frac": B_PAIR * value / world / 1e9 / HBM_PEAK_GBS},
                    "stage_ms_per_step_summed_over_groups": per_launch_ms,
                    "stage_ms_note": "per-stage table from a separate untimed single-chain pass with events at every stage boundary; launch_ms from the timed region; 'ingest' holds no launch (level 0 is the caller's image, read in place: what is left is the gap between two events); 'pyramid' = the resize launches alone for batches of 64 images and more (round 5: the blur of every level rides in FAST's launch, blur_levels_riding_in_launch; smaller batches blur beside the resize launches), 'blur' holds no launch; roofline.alg_bytes_per_launch = FAST's bytes + the riding levels' blur; ORBFE_NO_FUSE=1 separates them all"}
            roof["build_id"] = lib_build_id()
            roof["traffic_source"] = ("replayed from profiles/%s_traffic.json (rocprofv3 --pmc passes of this build: build ids match)" % PROFILE_ROUND) if roof["traffic"] else None
            if roof["traffic"]:
                roof["traffic_ratio"] = roof["traffic"] / roof["alg_bytes_per_launch"]  # counter bytes / algorithmic bytes of the dominant kernel
            wt, wsrc = whole_step_traffic_per_pair()
            if wt:
                roof["whole_pipeline"].update({"traffic_bytes_per_pair": wt, "traffic_ratio": wt / B_PAIR, "traffic_source": "profiles/" + wsrc})
            if _STALE:  # counter files of this round that were taken on another build: not replayed (their fields are null / absent)
                roof["stale_profile"] = True
                roof["stale_profiles"] = sorted(_STALE)
            if dom_alone is not None:
                roof["launch_ms_one_chain"] = dom_alone
                roof["frac_one_chain"] = alg[dom] * P / launches / (dom_alone * 1e-3) / 1e9 / HBM_PEAK_GBS
                roof["launch_ms_note"] = ("launch_ms: the kernel co-scheduled with the other %d chains' kernels (timed region); launch_ms_one_chain: the same "
                                          "launch with one chain at a time" % (C - 1))
        out = {
            "metric": metric, "value": value, "unit": "frames/s (1 frame = 1 stereo pair)",
            "n_gpus": ranks_joined, "steps": args.steps, "warmup": n_warm,
            "ms_per_step": step_ms, "higher_is_better": True, "scaling": args.mode,
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "Stereo-KITTI00-02 1241x376, 2000 features, 8 levels: extract L+R + ComputeStereoMatches"
                                   + (" (%d pairs per step per GPU, weak scaling)" % P if args.mode == "weak"
                                      else " (%d pairs per step in total, sharded round-robin over %d GPUs, strong scaling)" % (P_total, world)),
                       "sharding": args.mode, "pairs_per_step_per_gpu": P, "distinct_pairs": n_distinct, "chains_in_flight": C, "stream_groups": G,
                       "quadtree_kernel": ctx.quadtree_kernel(), "parallelism": "frame-pair sharding, no data-path collective",
                       "repeat": {"n": R, "min": pairs_per_step * args.steps / max(dts), "max": pairs_per_step * args.steps / min(dts), "value_is": "median"},
                       "keypoints_left_right_pair0": [int(counts[0]), int(counts[1])]},
        }
        if roof is not None:
            out["roofline"] = roof
        if piped is not None:
            pv = pairs_per_step * args.steps / piped[len(piped) // 2]
            out["config"]["pipelined"] = {"chains_in_flight": CP, "value": pv, "ms_per_step": piped[len(piped) // 2] / args.steps * 1e3,
                                          "min": pairs_per_step * args.steps / piped[-1], "max": pairs_per_step * args.steps / piped[0],
                                          "valu_issue_whole_step": (valu_issue(P, launches, dom_ms, piped[len(piped) // 2] / args.steps * 1e3) or {}).get("whole_step"),
                                          "note": "the same %d steps with %d step chains in flight (step k on context k %% %d and its stream), same barrier protocol, "
                                                  "median of %d; kernels of different chains share the chip, so per-kernel durations stretch (FAST ~2x) while the "
                                                  "whole-step issue fraction rises" % (args.steps, CP, CP, R)}
        if single is not None:
            out["config"]["one_chain_at_a_time"] = {"value": pairs_per_step * args.steps / single, "ms_per_step": single / args.steps * 1e3,
                                                    "note": "round 2's protocol (a step waits for the previous one's chain), median of 3"}
        if strong is not None:
            out["config"]["strong_scaling"] = strong
        if voc_blob is not None:
            out["config"]["vocabulary_broadcast_bytes"] = len(voc_blob)
        # what the collectives themselves saw: ranks = SUM all-reduce of 1 over the group (1 and "none" when no group exists)
        out["config"]["rccl"] = {"ranks": ranks_joined, "backend": args.backend if dist.is_initialized() else "none (single rank, no process group)",
                                 "broadcast_bytes": (len(params_blob) + 4096 + 32 + (len(voc_blob) + 8 + 32 if voc_blob is not None else 0)) if dist.is_initialized() else 0,
                                 "broadcasts": ["extractor parameters", "rBRIEF pattern (256 x 4 int32 + sha256)"] + (["vocabulary blob"] if voc_blob is not None else []),
                                 "self_launched": os.environ.get("ORBFE_BENCH_SELF_LAUNCHED") == "1"}
    for c in ctxs[1:]:
        c.close()
    if rank == 0:
        if args.full and world == 1 and args.small_batch > 0 and args.mode == "weak":
            out["config"]["small_batch"] = small_batch(api, torch, d_images, min(args.small_batch, P), make_ctx)
        if args.full and world == 1 and args.natural and args.mode == "weak":
            out["config"]["natural_image"] = natural_scene(api, torch, dev, P, make_ctx)
        if args.full and world == 1 and args.secondary and args.mode == "weak":
            try:
                out["config"]["secondary"] = secondary_configs(api, torch, dev)
                out["config"]["single_frame"] = single_frame(api, torch, dev)
            except Exception as e:  # an extra must not cost the headline its line
                out["config"]["secondary"] = {"error": repr(e)}
        if args.full and world == 1 and args.host_fed:
            out["config"]["host_fed"] = host_fed(api, torch, dev, host, P, make_ctx)
        if args.full and world == 1 and args.cpu_pairs > 0:
            out["cpu_baseline"] = cpu_baseline(args.cpu_pairs)
        else:
            out["cpu_baseline"] = None
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    ctx.close()
    if world > 1 or args.rehearse_rccl:
        D.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

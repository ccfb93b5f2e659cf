"""Shared pieces of bench.py (the headline + the driver's compact line) and bench_detail.py (the secondary lines): the synthetic
stream, the System session that replays it from HBM, and the stderr progress log."""
from __future__ import annotations

import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# The HIP runtime multiplexes all streams of a priority class onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams
# that share a queue serialise; the multi-session measurements drive up to 16 x 3 streams.  Must be set before HIP initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np
import torch

W, H, NKP = 640, 480, 2120          # C640: cell 12 -> 53 x 40 = 2120 keypoints
HBM_PEAK_GBS = 8000.0               # MI355X_MICROARCH.md: 8 TB/s spec
RING = 8                            # synthetic frames resident in HBM

STREAM_FRAMES = 200                  # frames of the synthetic stream resident in HBM (245 MB)
SYSTEM_CELL = 12                     # 53 x 40 = 2120 cells => ~2000 keypoints per frame


def stream_index(k: int) -> int:
    """frame k of the endless stream: the 200-frame crop sequence forwards, then backwards, ..."""
    period = 2 * (STREAM_FRAMES - 1)
    r = k % period
    return r if r < STREAM_FRAMES else period - r


class SystemJob:
    """The drop-in surface on one GPU: alva::System at cell 12 over a synthetic stream resident in HBM (and the same stream in host
    memory for the PCIe-fed variant).  width / height / cell default to configs[1]; --config 720p-streams runs configs[4]'s geometry
    (1280x720, cell 15 => 4080 cells) instead."""

    def __init__(self, device: int, seed: int, host_copy: bool = True, width: int = W, height: int = H, cell: int | None = None):
        from alvaar_amd import synth
        from alvaar_amd.system import AlvaAR
        self.dev = torch.device("cuda", device)
        cell = SYSTEM_CELL if cell is None else cell
        canvas = synth.texture_canvas(width, height, seed)
        host = np.stack([synth.gray_to_rgba(synth.frame_gray(canvas, k, width, height, noise_seed=11)) for k in range(STREAM_FRAMES)])
        self.frames = torch.from_numpy(host).to(self.dev)
        self.host_frames = host if host_copy else None
        self.ar = AlvaAR(width, height, device=device, cell_size=cell, random_sampling=False)
        self.k = -1
        self.status_hist = [0, 0, 0, 0]
        self.last_status = 0
        self.ptrs = [int(self.frames[i].data_ptr()) for i in range(STREAM_FRAMES)]

    def step(self):
        self.k += 1
        st = self.ar.find_camera_pose_device(self.ptrs[stream_index(self.k)], 33.0 * self.k)
        self.status_hist[st] += 1
        self.last_status = st
        return st == 1

    def step_ahead(self):
        """the same step with the NEXT frame named (alva_system_hint_next_frame_device): its gray image / pyramid are built beside this
        frame's pose solve"""
        self.k += 1
        st = self.ar.find_camera_pose_device(self.ptrs[stream_index(self.k)], 33.0 * self.k, self.ptrs[stream_index(self.k + 1)])
        self.status_hist[st] += 1
        return st == 1

    def step_host(self):
        self.k += 1
        # src/system.js:175 memImg.write(frame.data): AlvaAR.findCameraPose copies the caller's frame into its ONE registered frame buffer
        pose, st = self.ar.findCameraPose(self.host_frames[stream_index(self.k)], 33.0 * self.k)
        self.status_hist[st] += 1
        return st == 1

    def warm_to_steady_state(self, max_frames: int = 2500, then_untimed: int = 0):
        """Untimed: run until the map is in the regime a long session lives in -- the 30-keyframe window full (mapper.cpp:24-28 removes
        keyframe k - 30 from keyframe 31 on) -- then on to the middle of a keyframe period, so that a K-step window holds round(K / period)
        keyframes: the nearest whole number to their natural share.  Returns (frames run, keyframe period in frames)."""
        n0 = self.k
        kf_frames = []
        last = int(self.ar.state()[11])
        while self.k - n0 < max_frames:
            self.step()
            nk = int(self.ar.state()[11])
            if nk != last:
                kf_frames.append(self.k)
                last = nk
            if nk >= 34 and len(kf_frames) >= 8:
                break
        period = float(np.median(np.diff(kf_frames[-8:]))) if len(kf_frames) >= 3 else 0.0
        if period > 2:
            # the caller runs `then_untimed` more untimed steps (--warmup) before its window: aim so that the WINDOW starts mid-period
            target = int(period // 2 - then_untimed) % int(period)
            while (self.k - kf_frames[-1]) != target and self.k - n0 < max_frames + 64:
                self.step()
                nk = int(self.ar.state()[11])
                if nk != last:
                    kf_frames.append(self.k)
                    last = nk
        return self.k - n0, period


_T0 = time.perf_counter()


def log(msg: str):
    """progress on stderr (stdout carries the one JSON line)"""
    print(f"[bench {time.perf_counter() - _T0:7.2f}s] {msg}", file=sys.stderr, flush=True)



COMPACT_LIMIT = 4096


def _r(v, nd=4):
    """floats rounded to a few significant digits (the line is for a parser, the detail file keeps the full precision)"""
    if isinstance(v, float):
        return float(f"{v:.{nd + 2}g}")
    return v


def compact_line(full: dict) -> str:
    """The ONE stdout line of bench.py: the contract's keys + roofline + cpu_baseline + the few secondary figures the verdict asks for,
    guaranteed < 4 KB (round 3's 26 KB line overflowed the driver's stdout tail and was recorded as unparsed).  Missing sections are
    simply absent; if the object still came out too long the optional keys are dropped, longest first, never the contract's own."""
    import json
    g = full.get
    cfg = g("config", {})
    out = {k: _r(g(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                 "dtype", "data") if k in full}
    out["config"] = {k: _r(cfg[k]) for k in ("workload", "value_is", "keypoints_per_frame", "keyframe_period_frames", "parallelism") if k in cfg}
    for k in ("steps_timed", "seconds_timed", "keyframes_timed"):
        if k in full:
            out[k] = _r(full[k])
    if "value_window" in full:
        out["value_window"] = {k: _r(v) for k, v in full["value_window"].items() if k in ("frames_per_s", "steps", "keyframes", "value_over_window")}
    if "sustained" in full:
        out["sustained"] = {k: _r(v) for k, v in full["sustained"].items() if k in ("frames_per_s", "steps", "keyframes")}
    if "system_surface" in full:
        out["system_surface"] = {"frames_per_s": _r(full["system_surface"].get("frames_per_s"))}
    if "roofline" in full:
        out["roofline"] = {k: _r(v) for k, v in full["roofline"].items()
                           if k in ("kernel", "bound", "limiter", "achieved", "peak", "unit", "frac", "traffic", "alg_bytes_per_launch", "avg_us")}
    if "local_ba" in full:
        out["local_ba"] = {k: _r(v) for k, v in full["local_ba"].items()
                           if k in ("ms_per_solve", "residual_block_iters_per_s", "residual_blocks", "lm_iterations")}
        rb = g("roofline_ba", {})
        if "kernel_us_per_solve" in rb:
            out["local_ba"]["kernel_us_per_solve"] = _r(rb["kernel_us_per_solve"])
        gm = next((v for k, v in rb.get("kernels", {}).items() if k.startswith("k_gemm")), None)
        if gm:
            out["local_ba"]["mfma_f64"] = {"achieved_TFLOPs": gm.get("achieved_TFLOPs"), "peak_measured": gm.get("peak_TFLOPs_measured"),
                                           "frac_of_measured": _r(gm.get("frac_of_measured"))}
    if "cpu_baseline" in full:
        cb = full["cpu_baseline"]
        out["cpu_baseline"] = {k: _r(cb[k]) for k in ("value", "unit", "cores", "kind") if k in cb}
        out["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:260]
        if "eight_threads" in cb:
            out["cpu_baseline"]["eight_threads"] = {"value": _r(cb["eight_threads"].get("value")), "cores": 8}
        if "local_ba_ms" in cb:
            out["cpu_baseline"]["local_ba_ms"] = _r(cb["local_ba_ms"])
    fs = g("frame_sections_us", {})
    if "ms_per_keyframe" in fs:
        out["ms_per_keyframe"] = fs["ms_per_keyframe"]
    # secondary figures measured before the line is printed (bench.py, run_secondary(part="line")): flat keys
    g32 = g("system_group32") or {}
    if "frames_per_s" in g32:
        out["group32_frames_per_s"] = _r(g32["frames_per_s"])
        if g32.get("ms_keyframe_step_mean") is not None:
            out["group32_ms_keyframe_step"] = _r(g32["ms_keyframe_step_mean"])
    s720 = g("system_720p") or {}
    if "frames_per_s" in s720:
        out["system_720p_frames_per_s"] = _r(s720["frames_per_s"])
        if "ms_per_keyframe" in s720:
            out["system_720p_ms_per_keyframe"] = _r(s720["ms_per_keyframe"])
    c720 = g("config_1280x720") or {}
    if "ms_per_frame" in c720:
        out["orb720_us_per_frame"] = _r(1e3 * c720["ms_per_frame"])
        fn = (c720.get("kernels") or {}).get("k_fast_nms") or {}
        if "GBps" in fn:
            out["orb720_k_fast_nms_GBps"] = _r(fn["GBps"])
    bd = g("bounds", {}).get("inputs", {})
    if "tracking_chain_kernel_us" in bd:
        out["tracking_chain"] = {"launches": bd.get("launches_on_the_tracking_chain"), "kernel_us": _r(bd["tracking_chain_kernel_us"])}
    mm = g("map_merge") or {}
    if mm and "error" not in mm:
        out["map_merge"] = {k: _r(mm[k]) for k in ("backend", "world", "records_gathered", "fused", "applied", "all_gather_us", "fuse_us") if k in mm}
    if "detail_file" in full:
        out["detail_file"] = full["detail_file"]
    optional = ["sustained", "map_merge", "tracking_chain", "orb720_k_fast_nms_GBps", "group32_ms_keyframe_step", "system_720p_ms_per_keyframe", "ms_per_keyframe", "system_surface", "steps_timed", "seconds_timed", "keyframes_timed", "value_window", "local_ba"]
    line = json.dumps(out, separators=(",", ":"))
    while len(line) >= COMPACT_LIMIT and optional:
        out.pop(optional.pop(0), None)
        line = json.dumps(out, separators=(",", ":"))
    if len(line) >= COMPACT_LIMIT:      # only the contract's keys are left: shorten the two free-text fields
        out["config"]["workload"] = out["config"].get("workload", "")[:200]
        if "cpu_baseline" in out:
            out["cpu_baseline"]["sample"] = out["cpu_baseline"]["sample"][:80]
        line = json.dumps(out, separators=(",", ":"))
    assert len(line) < COMPACT_LIMIT, len(line)
    return line

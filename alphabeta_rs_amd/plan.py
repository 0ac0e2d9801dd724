"""abn_plan and abn_multi: the device-resident batch of fits on one GPU and on several, and the host arithmetic beside
them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import FIT_INFO_DTYPE, KERNEL_NAMES, AbnError, Options, _arr, _dev, _f64, _Handle, _ok, _opt, _ptr, load_library
from .context import Context


class _FitPlan(_Handle):
    """What Plan and MultiPlan share, entry point for entry point (`_PREFIX`: abn_plan / abn_multi): W windows x (S
    starts + B bootstraps) over N rows."""

    def set_window_ids(self, ids):
        """ids[W]: every window's index in the Philox counters (default window_offset + w); before set_windows"""
        a = None if ids is None else _arr(ids, np.uint32, self.W)
        self._check(self._entry("set_window_ids")(self._h, _ptr(a)))

    def set_windows(self, d_obs, p0uu, eqp=None, eqp_weight=None):
        d = _f64(d_obs, (self.W, self.N))
        p = _f64(p0uu, (self.W,))
        e = None if eqp is None else _f64(eqp, (self.W,))
        ew = None if eqp_weight is None else _f64(eqp_weight, (self.W,))
        self._check(self._entry("set_windows")(self._h, _ptr(d), _ptr(p), _ptr(e), _ptr(ew)))

    def set_stream_sweep(self, mode: int):
        """0 (default): streamed chains re-read their rows every cost evaluation; 1: once per Nelder-Mead iteration
        (reflection, expansion and contraction in one pass) where the launch streams with a wavefront per chain — same
        bytes either way"""
        self._check(self._entry("set_stream_sweep")(self._h, mode))

    def run(self):
        self._check(self._entry("run")(self._h))

    def sync(self):
        self._check(self._entry("sync")(self._h))

    def _kernel_ms(self, *device_index):
        ms = self._ms(self._entry("kernel_ms"), 3, *device_index)
        return {"fit_starts": ms[0], "select": ms[1], "fit_boot": ms[2]}

    def _download(self, want_info, allow_failed_windows, with_a, with_b):
        W, N, S, B = self.W, self.N, self.S, self.B
        models, pred, resid = np.empty((W, 4)), np.empty((W, N)), np.empty((W, N))
        raw = np.empty((W, B, 7)) if with_b else None
        ia = np.zeros((W, S), dtype=FIT_INFO_DTYPE) if (with_a and want_info) else None
        ib = np.zeros((W, B), dtype=FIT_INFO_DTYPE) if (with_b and want_info) else None
        bs = np.full(W, -1, dtype=np.int32)
        rc = self._entry("download")(self._h, _ptr(models), _ptr(pred), _ptr(resid), _ptr(raw), _ptr(ia), _ptr(ib),
                                     _ptr(bs))
        if not (rc == 5 and allow_failed_windows):  # ABN_ERR_NO_FINITE_FIT: every buffer is filled all the same
            self._check(rc)
        return {"models": models, "pred": pred, "resid": resid, "raw": raw, "info_a": ia, "info_b": ib,
                "best_start": bs}

    def analyze(self, allow_failed_windows=False):
        """The analysis of every window on the device, from the table the plan currently writes (bind_raw included):
        (out (W, 32), first_bad (W,)) as analyze_batch — W x 32 doubles come back instead of raw (W, B, 7).  MultiPlan:
        Plan.analyze for all W windows, on the first device's gathered table."""
        out, fb = np.empty((self.W, 32)), np.full(self.W, -1, dtype=np.int32)
        rc = self._entry("analyze")(self._h, _ptr(out), _ptr(fb))
        if not (rc == 5 and allow_failed_windows):
            self._check(rc)
        return out, fb

    def counters(self):
        out = (C.c_int64 * 5)()
        self._check(self._entry("counters")(self._h, out))
        return {"fits": out[0], "evals": out[1], "iters": out[2], "evals_skipped": out[3] + out[4],
                "evals_skipped_starts": out[3], "evals_skipped_boot": out[4]}


class Plan(_FitPlan):
    """abn_plan: device-resident batch of W windows x (S starts + B bootstraps) over one pedigree topology."""

    _DESTROY, _PREFIX = "abn_plan_destroy", "abn_plan"

    def __init__(self, ctx: Context, generations, n_windows, n_starts, n_boot, *, window_offset=0, boot_offset=0,
                 options: Options | None = None):
        self.ctx = ctx
        self._L = ctx._L
        g = _f64(generations).reshape(-1, 3)
        self.N, self.W, self.S, self.B = g.shape[0], n_windows, n_starts, n_boot
        h = C.c_void_p()
        self._check(self._L.abn_plan_create(ctx._h, _opt(options), _ptr(g), self.N, n_windows, n_starts, n_boot,
                                            window_offset, boot_offset, C.byref(h)))
        self._h = h

    def failed_windows(self) -> int:
        """windows whose selection found no finite start in the last phase-A run"""
        n = C.c_int32(0)
        self._check(self._L.abn_plan_failed_windows(self._h, C.byref(n)))
        return n.value

    def run_phase(self, phase: int):
        self._check(self._L.abn_plan_run_phase(self._h, phase))

    def tail_handed(self):
        """chains the last persistent launch of (phase A, phase B) handed to the speculative kernel for its tail"""
        out = (C.c_int64 * 2)()
        self._check(self._L.abn_plan_tail_handed(self._h, out))
        return int(out[0]), int(out[1])

    def set_early_bootstraps(self, mode: int):
        """0: run() launches phase B after the slowest start; 1 (default): on a quorum of the starts where the plan is
        eligible (one window, >= 5 starts on the speculative kernel, bootstraps on the persistent kernel)"""
        self._check(self._L.abn_plan_set_early_bootstraps(self._h, mode))

    def early_bootstraps(self):
        """the plan's eligibility and quorum; starts parked at the quorum and the miss flag of the last run()"""
        out = (C.c_int32 * 4)()
        self._check(self._L.abn_plan_early_bootstraps(self._h, out))
        return {"eligible": bool(out[0]), "quorum": int(out[1]), "parked": int(out[2]), "miss": bool(out[3])}

    def stream_sweep(self):
        """the mode; whether the last run of each phase used the sweep kernel; passes over the rows those launches counted"""
        out = (C.c_int64 * 4)()
        self._check(self._L.abn_plan_stream_sweep(self._h, out))
        return {"mode": int(out[0]), "starts": bool(out[1]), "boot": bool(out[2]), "passes": int(out[3])}

    def kernel_ms(self):
        return self._kernel_ms()

    def raw_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._L.abn_plan_raw_device_ptr(self._h, C.byref(p)))
        return p.value or 0

    def bind_raw(self, dev_ptr: int):
        self._check(self._L.abn_plan_bind_raw(self._h, _dev(dev_ptr)))

    def download(self, want_info=True, allow_failed_windows=False):
        """Raises AbnError(ABN_ERR_NO_FINITE_FIT) when a window has no finite start (the reference panics) unless
        allow_failed_windows: then the dict comes back with best_start = -1 and NaN rows for those windows."""
        return self._download(want_info, allow_failed_windows, self.S, self.B)   # an empty phase: None

    def device_bytes(self) -> int:
        b = C.c_int64()
        self._check(self._L.abn_plan_device_bytes(self._h, C.byref(b)))
        return b.value

    def last_kernels(self):
        """which fit kernel the last run of each phase used (ABN_KERNEL_* names) and its lanes per chain"""
        out = (C.c_int32 * 4)()
        self._check(self._L.abn_plan_last_kernels(self._h, out))
        return {"starts": (KERNEL_NAMES.get(out[0], out[0]), out[1]), "boot": (KERNEL_NAMES.get(out[2], out[2]), out[3])}


def reduction_tree(generations, options: Options | None = None) -> int:
    """The residual reduction tree of a pedigree (abn_fit_info.lanes): host arithmetic, no device needed."""
    g = _f64(generations).reshape(-1, 3)
    t = C.c_int32(0)
    _ok(load_library().abn_reduction_tree(_opt(options), _ptr(g), g.shape[0], C.byref(t)))
    return t.value


def multi_plan_shard(n_windows: int, n_boot: int, n_devices: int, device_index: int):
    """(window_offset, n_windows, boot_offset, n_boot) of one device's shard in the one-process / several-GPUs entry
    points (abn_multi_plan_shard: host arithmetic, no device needed)."""
    out = (C.c_int32 * 4)()
    _ok(load_library().abn_multi_plan_shard(n_windows, n_boot, n_devices, device_index, out))
    return tuple(int(v) for v in out)


def rccl_available() -> bool:
    ok = C.c_int(0)
    load_library().abn_multi_rccl_available(C.byref(ok))
    return bool(ok.value)


class MultiPlan(_FitPlan):
    """abn_multi: one process, several GPUs — a plan per device, windows (or, with fewer windows than devices,
    bootstraps) sharded in contiguous blocks, the bootstrap tables gathered with RCCL over xGMI."""

    _DESTROY, _PREFIX = "abn_multi_destroy", "abn_multi"

    def __init__(self, devices, generations, n_windows, n_starts, n_boot, *, options: Options | None = None):
        self._L = load_library()
        g = _f64(generations).reshape(-1, 3)
        self.devices = [int(d) for d in devices]
        self.N, self.W, self.S, self.B = g.shape[0], n_windows, n_starts, n_boot
        devs = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        rc = self._L.abn_multi_create(devs, len(self.devices), _opt(options), _ptr(g), self.N, n_windows, n_starts,
                                      n_boot, C.byref(h))
        self._h = h if h.value else None
        if rc:
            msg = (self._L.abn_multi_last_error(h) or b"").decode() if h.value else ""
            self.close()
            raise AbnError(rc, msg)

    def _check(self, rc):
        if rc:
            raise AbnError(rc, (self._L.abn_multi_last_error(self._h) or b"").decode())

    def kernel_ms(self, device_index: int = 0):
        return self._kernel_ms(device_index)

    def shard(self, device_index: int):
        out = (C.c_int32 * 4)()
        self._check(self._L.abn_multi_shard(self._h, device_index, out))
        return {"window_offset": out[0], "n_windows": out[1], "boot_offset": out[2], "n_boot": out[3]}

    def download(self, want_info=True, allow_failed_windows=False):
        return self._download(want_info, allow_failed_windows, True, True)   # every array, whatever B and S are

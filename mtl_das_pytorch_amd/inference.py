"""Sliding-window inference over long DAS recordings.

A recording is a (fiber position x time) matrix, usually much larger than the 100 x 250 window the
models are trained on.  It is cut into windows with a configurable stride; the windows are sharded over
the data-parallel ranks, evaluated, and the per-window predictions (distance bin, event type and class
probabilities) are gathered on every rank.  This is batch growth, served by data parallelism, not a
sequence-parallel scheme (there is no sequence dimension in these models).

Execution: on a GPU the window batches run through the lowered HIP engine's eval program (bf16 MFMA,
BN with running statistics, one HIP graph per batch); elsewhere through the PyTorch module in fp32.

On the engine path the recording is resident (``windows="resident"``): it is uploaded once, the batch's windows
are cut on the device straight into the stem's input, the probabilities land in a resident table from inside the
graph, and the window stack -- (100 * 250) / (stride_f * stride_t) times the recording -- never exists.
:func:`prediction_map` averages the overlapping windows' probabilities into an event-probability and distance
map along the fiber over time.

The models have no "nothing is happening" class.  ``predict_recording(gate_db=...)`` puts an energy detector in front
of them: the windows' power is measured (on the engine path on the device, csrc/gate.hip), those below the noise
floor by the gate are reported as quiet and only the others are evaluated.

:class:`LiveRecording` serves a recording that is still growing: chunks of time samples go into a ring, the windows
that became available are evaluated by replays of one graph, and map columns are returned as they become final
(csrc/live.hip on the engine path, a host ring and the fp32 module elsewhere).  ``LiveRecording(gate_db=...)`` gates
the stream too: its noise floor runs along with it (:func:`running_floor_reference`; csrc/live_gate.hip).

A recording at the interrogator's raw rate (``decimate=D``, fp32 or int16) is low-pass filtered and decimated first
(data/resample.py is the definition; csrc/resample.hip on the engine path): :func:`decimate_recording` for a whole
recording, and in :class:`LiveRecording` piece by piece with the filter's state carried across the pushes, so the
decimated stream does not depend on how the raw one was cut.

``common_mode="median" | "mean"`` subtracts, per time sample, the lower median or the mean over the fiber from the
stream the windows are cut from -- the common mode, which would otherwise open the gate on the whole fiber
(data/common_mode.py is the definition; csrc/common_mode.hip on the engine path): :func:`remove_common_mode` for a
whole recording, and in :class:`LiveRecording` on every chunk before it enters the ring.  Time columns are
independent, so no state is carried and the cut of a stream does not matter.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .models import decode_joint
from .parallel.dist import DistContext

WINDOW = (100, 250)


def window_starts(length: int, win: int, stride: int) -> np.ndarray:
    """Window start offsets covering ``[0, length)``; the last window is aligned to the end so every
    sample is covered (no partial windows)."""
    if length < win:
        raise ValueError(f"recording dimension {length} is shorter than the window {win}")
    starts = list(range(0, length - win + 1, stride))
    if starts[-1] != length - win:
        starts.append(length - win)
    return np.asarray(starts, dtype=np.int64)


def sliding_windows(rec: torch.Tensor, window: Tuple[int, int] = WINDOW, stride: Tuple[int, int] = (100, 125)):
    """``rec``: [F, T] or [C, F, T].  Returns (tiles [N, C, wf, wt], positions [N, 2] = (f0, t0))."""
    if rec.dim() == 2:
        rec = rec.unsqueeze(0)
    C, Fn, Tn = rec.shape
    fs, ts = window_starts(Fn, window[0], stride[0]), window_starts(Tn, window[1], stride[1])
    tiles = rec.unfold(1, window[0], 1).unfold(2, window[1], 1)  # [C, F', T', wf, wt] (views)
    sel = tiles[:, fs][:, :, ts]                                      # [C, nf, nt, wf, wt]
    out = sel.permute(1, 2, 0, 3, 4).reshape(len(fs) * len(ts), C, window[0], window[1]).contiguous()
    pos = np.stack(np.meshgrid(fs, ts, indexing="ij"), -1).reshape(-1, 2)
    return out, pos


def _shard(n: int, ctx: Optional[DistContext]) -> Tuple[int, int]:
    if ctx is None or not ctx.enabled:
        return 0, n
    per = (n + ctx.world - 1) // ctx.world
    return min(n, ctx.rank * per), min(n, (ctx.rank + 1) * per)


def _recording_windows(rec: torch.Tensor, stride, ctx: Optional[DistContext]):
    """What every form of :func:`predict_recording` starts from: the recording as fp32 [C, F, T], its window starts
    ``fs`` / ``ts``, the positions [N, 2] of its N windows (window ``n = a * len(ts) + b`` at ``(fs[a], ts[b])``, the
    order of :func:`sliding_windows`), N and this rank's shard ``(lo, hi)`` of them."""
    rec3 = rec.float().unsqueeze(0) if rec.dim() == 2 else rec.float()
    fs, ts = window_starts(rec3.shape[1], WINDOW[0], stride[0]), window_starts(rec3.shape[2], WINDOW[1], stride[1])
    pos = np.stack(np.meshgrid(fs, ts, indexing="ij"), -1).reshape(-1, 2)
    return rec3, fs, ts, pos, len(pos), _shard(len(pos), ctx)


def _torch_probs(model: nn.Module, model_type: str, x: torch.Tensor) -> Sequence[torch.Tensor]:
    out = model(x)
    if model_type == "multi_classifier":
        return [torch.softmax(out[0] if isinstance(out, tuple) else out, 1)]
    outs = out if isinstance(out, tuple) else (out,)
    return [o.exp() for o in outs]  # A/B heads emit log-probabilities


def window_power_reference(rec, fs, ts, window: Tuple[int, int] = WINDOW) -> np.ndarray:
    """fp64 power [len(fs) * len(ts)] of the windows of ``rec`` ([F, T] or [C, F, T]; window ``n = a * len(ts) + b``
    at ``(fs[a], ts[b])``): the mean over the channels of the mean over the window of ``(x - mu_c)^2``, ``mu_c``
    the window's own mean in channel ``c`` -- the power of data/noise.py applied to a window.  This is the
    definition; csrc/gate.hip evaluates it on the device."""
    x = rec.detach().cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    x = x.astype(np.float64)
    if x.ndim == 2:
        x = x[None]
    out = np.empty((len(fs), len(ts)))
    for a, f0 in enumerate(fs):
        for b, t0 in enumerate(ts):
            w = x[:, int(f0):int(f0) + window[0], int(t0):int(t0) + window[1]]
            out[a, b] = ((w - w.mean((1, 2), keepdims=True)) ** 2).mean()  # equal planes: the mean of the means
    return out.reshape(-1)


def _auto_floor(noise_floor) -> bool:
    """``noise_floor`` of :func:`predict_recording`: True for ``"auto"``, False for a power; no other string."""
    if isinstance(noise_floor, str) and noise_floor != "auto":
        raise ValueError(f"noise_floor must be 'auto' or a power, got {noise_floor!r}")
    return isinstance(noise_floor, str)


def noise_floor_reference(power: np.ndarray, nt: int, noise_floor="auto") -> np.ndarray:
    """The noise floor of every fiber start, fp64 [nf]: a number is one floor for all of them; ``"auto"`` is the lower
    median over time of the start's window powers, ``sorted(power[a, :])[(nt - 1) // 2]`` (noise varies along a
    fiber, and an event is short against a recording)."""
    p = np.asarray(power, dtype=np.float64).reshape(-1, nt)
    if _auto_floor(noise_floor):
        return np.sort(p, 1)[:, (nt - 1) // 2]
    return np.full(len(p), float(noise_floor))


def active_reference(power: np.ndarray, nt: int, gate_db: float, noise_floor="auto") -> np.ndarray:
    """The gate's flags in fp64, bool [N]: window ``n`` is active unless its power is below the floor of its fiber
    start times ``10^(gate_db / 10)``; a NaN power is active (never hidden)."""
    p = np.asarray(power, dtype=np.float64)
    thr = np.repeat(noise_floor_reference(p, nt, noise_floor), nt) * 10.0 ** (float(gate_db) / 10.0)
    return ~(p < thr)


def running_floor_reference(power, nf: int, history: int, warmup: int) -> np.ndarray:
    """The noise floor that runs along with a stream, fp64 [nj, nf], of the window powers ``power`` [nj * nf] in live
    numbering (``n = j * nf + a``).  Causal: with ``lo = max(0, j - history + 1)`` and ``m = j - lo + 1``,

        floor[j, a] = sorted(power[lo .. j, a])[(m - 1) // 2]

    the lower median of the last ``m <= history`` powers of fiber start ``a``, row ``j`` itself included and no row
    after it, NaN ordered last as ``np.sort`` does; 0 -- "no floor yet", under which every window is active -- while
    ``m < warmup``.  This is the definition; csrc/live_gate.hip evaluates it on the device.

    A trailing median follows a level that persists: an event longer than about ``history / 2`` time indices
    becomes the floor and fades from the flags.  (A floor that freezes while windows are active would depend on the
    flags it decides, and is not what this is.)"""
    if history < 1 or not 1 <= warmup <= history:
        raise ValueError(f"1 <= warmup <= history, got warmup {warmup}, history {history}")
    p = np.asarray(power, dtype=np.float64).reshape(-1, nf)
    floor = np.zeros_like(p)
    for j in range(len(p)):
        lo = max(0, j - history + 1)
        m = j - lo + 1
        if m >= warmup:
            floor[j] = np.sort(p[lo:j + 1], 0)[(m - 1) // 2]
    return floor


def live_active_reference(power, floor, gate_db: float) -> np.ndarray:
    """The live gate's flags in fp64, bool like ``power``: active unless the power is below its own floor times
    ``10^(gate_db / 10)`` -- a floor of 0 and a NaN power are active (nothing is hidden before the floor exists)."""
    p, f = np.asarray(power, dtype=np.float64), np.asarray(floor, dtype=np.float64)
    return ~(p < f.reshape(p.shape) * 10.0 ** (float(gate_db) / 10.0))


def _power_db(power: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.asarray(power, dtype=np.float64))


def _raw_recording(rec) -> torch.Tensor:
    """A raw recording or chunk as a tensor [C, F, T]: int16 stays int16, anything else becomes fp32."""
    raw = torch.as_tensor(rec)
    if raw.dim() == 2:
        raw = raw.unsqueeze(0)
    if raw.dim() != 3:
        raise ValueError(f"a recording is [F, T] or [C, F, T], got {tuple(raw.shape)}")
    return raw if raw.dtype == torch.int16 else raw.float()


def _decimation(decimate, taps):
    """``(D, taps)`` of a ``decimate`` / ``taps`` argument pair, the taps as the fp32 [L] array the filter runs
    with; ``(None, None)`` without decimation."""
    if decimate is None:
        if taps is not None:
            raise ValueError("taps without decimate")
        return None, None
    from .data.resample import as_taps
    h = as_taps(taps, decimate)
    return int(decimate), h


def _raw_times(res: Dict, D: int, L: int, Wt: int = WINDOW[1]) -> Dict:
    """The windows' extent in raw samples: ``raw_time_start`` and ``raw_time_stop``, one past the last raw sample
    the window depends on."""
    t0 = res["positions"][:, 1]
    res["raw_time_start"], res["raw_time_stop"] = t0 * D, (t0 + Wt - 1) * D + L
    return res


@torch.no_grad()
def decimate_recording(rec, D: int, taps=None, device=None, use_engine: Optional[bool] = None) -> torch.Tensor:
    """The raw recording ``rec`` ([F, T] or [C, F, T], fp32 or int16) through the FIR ``taps`` (None:
    ``data.resample.decimation_taps(D)``) and decimation by ``D``: fp32 [C, F, K], ``K = (T - L) // D + 1`` (the
    "valid" form of data/resample.py: no padded edge).  On the engine path the raw recording is uploaded as it is
    (int16 stays int16), one ``fir_decimate`` launch runs on it and the result stays on the device; elsewhere the
    fp64 reference, rounded to fp32."""
    if D is None:
        raise ValueError("decimate_recording needs a factor D")
    D, h = _decimation(D, taps)
    raw = _raw_recording(rec)
    device = torch.device(device) if device is not None else raw.device
    if use_engine is None:
        use_engine = device.type == "cuda"
    if use_engine:
        from .ops import functional as HF
        raw_d = raw.to(device).contiguous()
        return HF.fir_decimate(raw_d, None, 0, 0, torch.from_numpy(h).to(device), D)[0]
    from .data.resample import fir_decimate_reference
    return torch.from_numpy(fir_decimate_reference(raw.cpu().numpy(), h, D).astype(np.float32)).to(device)


def _model_rate_recording(rec) -> torch.Tensor:
    """A recording or chunk at the model's rate as an fp32 tensor [C, F, T]; int16 is the raw rate's type and is
    refused."""
    x = torch.as_tensor(rec)
    if x.dtype == torch.int16:
        raise ValueError("an int16 recording is at the raw rate: it needs decimate")
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError(f"a recording is [F, T] or [C, F, T], got {tuple(x.shape)}")
    return x.float()


def _remove_common_mode(x: torch.Tensor, how: str, device, use_engine: bool, own: bool):
    """:func:`remove_common_mode` of the fp32 [C, F, T] tensor ``x``; ``own``: ``x`` is a copy of the caller's data
    that may be overwritten."""
    if use_engine:
        from .ops import functional as HF
        x_d = x.to(device).contiguous()
        own = own or x_d.data_ptr() != x.data_ptr()  # the upload or the repacking made a copy
        return HF.common_mode(x_d, how, out=x_d if own else None)
    from .data.common_mode import common_mode_reference
    y, m = common_mode_reference(x.detach().cpu().numpy(), how)
    return torch.from_numpy(y).to(device), torch.from_numpy(m).to(device)


@torch.no_grad()
def remove_common_mode(rec, how: str = "median", device=None, use_engine: Optional[bool] = None):
    """The recording ``rec`` ([F, T] or [C, F, T], at the model's rate) minus its common mode: per channel and time
    sample the lower median (``how="median"``) or the mean (``"mean"``) over the fiber (data/common_mode.py is the
    definition).  Returns ``(clean [C, F, T] fp32, trace [C, T] fp32)``, ``trace`` the value subtracted.  On the
    engine path the recording is uploaded, one ``common_mode`` launch runs on it and the result stays on the device,
    with the definition's bits; elsewhere the reference.  A device tensor passed in is never modified (a copy this
    function made itself is cleaned in place).  The estimate is over the whole fiber; a sub-range is not offered."""
    from .data.common_mode import as_common_mode
    how = as_common_mode(how)
    if how is None:
        raise ValueError("remove_common_mode needs 'median' or 'mean'")
    raw = torch.as_tensor(rec)
    x = _model_rate_recording(raw)
    device = torch.device(device) if device is not None else x.device
    if use_engine is None:
        use_engine = device.type == "cuda"
    return _remove_common_mode(x, how, device, use_engine, own=x.data_ptr() != raw.data_ptr())


@torch.no_grad()
def predict_recording(model: nn.Module, model_type: str, rec: torch.Tensor, stride=(100, 125), batch: int = 32,
                      ctx: Optional[DistContext] = None, device=None, use_engine: Optional[bool] = None,
                      windows: Optional[str] = None, runner=None, gate_db: Optional[float] = None,
                      noise_floor="auto", decimate: Optional[int] = None, taps=None,
                      common_mode: Optional[str] = None) -> Dict:
    """Per-window predictions for one recording.  Returns numpy arrays: ``positions`` [N, 2], and per task
    (``distance`` / ``event`` as the model provides) ``<task>_pred`` [N] and ``<task>_prob`` [N, k].

    ``windows``: ``"resident"`` (the engine path's default) uploads the recording once and cuts the windows on
    the device; ``"materialize"`` (the torch backend's only form) builds the window stack on the host.
    ``runner``: a :func:`window_runner` of this model to reuse over many recordings (resident windows only; its
    batch size holds); without one the call lowers the model itself.

    ``gate_db``: an energy detector in front of the model, which has no "nothing is happening" class.  A window is
    active unless its power (:func:`window_power_reference`) is below ``noise_floor`` times ``10^(gate_db / 10)``;
    only active windows are evaluated.  ``noise_floor``: a power, or ``"auto"``: per fiber start the lower median
    of its windows' powers over time.  The result gains ``active`` [N] bool and ``power_db`` [N]; a quiet window has
    ``<task>_pred`` -1 (Model C's decoded ``distance_pred`` / ``event_pred`` too) and a zero ``<task>_prob`` row.
    On the resident path power, floor, selection and the evaluation of the selected windows run on the device
    (csrc/gate.hip); every rank computes all flags and gates its own shard.  None: no gate, every window
    evaluated.

    ``decimate`` = D: ``rec`` is at the raw rate (fp32 or int16) and goes through :func:`decimate_recording` with
    ``taps`` first; everything else runs on the result as it does without, every rank decimating for itself.  The
    result gains ``raw_time_start`` = ``positions[:, 1] * D`` and ``raw_time_stop`` =
    ``(positions[:, 1] + Wt - 1) * D + L``, one past the last raw sample the window depends on.  None: ``rec`` is at
    the model's rate.

    ``common_mode`` = ``"median"`` or ``"mean"``: :func:`remove_common_mode` is applied to the stream the windows
    are cut from -- with ``decimate`` that is the decimated recording, after the FIR: fp32, and D times fewer columns
    -- and gate, selection, windows and maps run unchanged on the result, every rank cleaning for itself as it
    decimates for itself.  The mean commutes with the FIR (both are linear, up to rounding); the median does not:
    the median of the decimated recording is what is removed, not the decimated median of the raw one.  An int16
    recording without ``decimate`` is an error.  None: nothing is removed."""
    device = torch.device(device) if device is not None else (ctx.device if ctx else torch.device("cpu"))
    if use_engine is None:
        use_engine = device.type == "cuda"
    D, h = _decimation(decimate, taps)
    from .data.common_mode import as_common_mode
    how = as_common_mode(common_mode)
    if D is not None or how is not None:
        own = D is not None  # the decimated recording is this call's own
        front = decimate_recording(rec, D, h, device, use_engine) if own else _model_rate_recording(rec)
        if how is not None:
            front = _remove_common_mode(front, how, device, use_engine, own)[0]
        res = predict_recording(model, model_type, front, stride, batch, ctx, device, use_engine, windows, runner,
                                gate_db, noise_floor)
        return _raw_times(res, D, len(h)) if D is not None else res
    if windows is None:
        windows = "resident" if use_engine else "materialize"
    if windows not in ("resident", "materialize"):
        raise ValueError(f"windows must be 'resident' or 'materialize', got {windows!r}")
    if windows == "resident" and not use_engine:
        raise ValueError("windows='resident' needs the engine backend")
    if runner is not None and windows != "resident":
        raise ValueError("a window runner serves windows='resident' only")
    names, ncls = _task_names(model, model_type)
    rec3, fs, ts, pos, n, (lo, hi) = _recording_windows(rec, stride, ctx)
    if windows == "resident":
        gate = None if gate_db is None else (float(gate_db), noise_floor)
        if runner is not None:
            table = resident_probs(runner, rec3, fs, ts, lo, hi, gate=gate)
        else:
            table = _resident_probs(model, model_type, rec3, fs, ts, lo, hi, batch, device, gate)
        flags = None
        if gate is not None:
            table, active, power = table
            flags = (active.cpu().numpy().astype(bool), power.cpu().numpy())
        probs = [p.contiguous() for p in table.split(ncls, 1)]
        return _result(model_type, names, probs, pos, ctx, flags)
    flags = None
    if gate_db is not None:
        # the same gate by the fp64 reference; only the active windows of this rank's shard are stacked
        power = window_power_reference(rec3, fs, ts)
        flags = (active_reference(power, len(ts), gate_db, noise_floor), power)
        keep = lo + np.flatnonzero(flags[0][lo:hi])
        rows = torch.from_numpy(keep).to(device)
        mine = torch.zeros(0)
        if len(keep):
            mine = torch.stack([rec3[:, f0:f0 + WINDOW[0], t0:t0 + WINDOW[1]] for f0, t0 in pos[keep]]).to(device)
    else:
        rows = slice(lo, hi)
        mine = sliding_windows(rec3, stride=stride)[0][lo:hi].to(device)
    probs = [torch.zeros(n, k, device=device) for k in ncls]
    if len(mine):
        if use_engine:
            chunks = _engine_probs(model, model_type, mine, batch, device)
        else:
            model.eval().to(device)
            chunks = [[] for _ in names]
            for i in range(0, len(mine), batch):
                for t, p in enumerate(_torch_probs(model, model_type, mine[i:i + batch])):
                    chunks[t].append(p)
            chunks = [torch.cat(c) for c in chunks]
        for t in range(len(names)):
            probs[t][rows] = chunks[t].float()
    return _result(model_type, names, probs, pos, ctx, flags)


def _result(model_type: str, names, probs, pos, ctx: Optional[DistContext], flags=None) -> Dict:
    """The result dict from the per-task probability tables (each rank filled its own rows of a zeroed table).
    ``flags``: a gated call's (active [N] bool, power [N]), the same on every rank: quiet windows predict -1."""
    if ctx is not None and ctx.enabled:  # every rank wrote its own rows; the sum is the gather
        for p in probs:
            ctx.all_reduce_(p)
    res = {"positions": pos}
    if model_type == "multi_classifier":
        joint = probs[0].argmax(1)
        d, e = decode_joint(joint)
        res.update(joint_pred=joint.cpu().numpy(), joint_prob=probs[0].cpu().numpy(), distance_pred=d.cpu().numpy(),
                   event_pred=e.cpu().numpy())
    else:
        for t, name in enumerate(names):
            res[f"{name}_pred"] = probs[t].argmax(1).cpu().numpy()
            res[f"{name}_prob"] = probs[t].cpu().numpy()
    if flags is not None:
        active, power = flags
        for k in [k for k in res if k.endswith("_pred")]:
            res[k] = np.where(active, res[k], -1)
        res["active"], res["power_db"] = active, _power_db(power)
    return res


def _engine_probs(model: nn.Module, model_type: str, x: torch.Tensor, batch: int, device) -> Sequence[torch.Tensor]:
    """Eval-mode forward of the lowered program over window batches (the last batch padded)."""
    from .engine.step import StepRunner
    n = len(x)
    prog = _eval_program(model, model_type, batch, device, tuple(x.shape[2:]))
    labels = torch.zeros((n,) if model_type == "multi_classifier" else (n, 2), dtype=torch.int64, device=device)
    runner = StepRunner(prog, x, labels, use_graph=True, X_eval=x, labels_eval=labels)
    outs = [[] for _ in range(1 if model_type == "multi_classifier" else prog.T)]
    for i in range(0, n, batch):
        idx = torch.arange(i, min(n, i + batch), device=device)
        m = idx.numel()
        if m < batch:
            idx = torch.cat([idx, idx[:1].expand(batch - m)])
        runner.eval_step(idx)
        if model_type == "multi_classifier":
            outs[0].append(torch.softmax(prog.logp[:m], 1).clone())
        else:
            for t in range(prog.T):
                k = 16 if prog.lab_off[t] == 0 else 2
                outs[t].append(prog.logp[t, :m, :k].exp().clone())
    return [torch.cat(o) for o in outs]


def _eval_program(model: nn.Module, model_type: str, batch: int, device, in_hw):
    """The lowered program of ``model`` for inputs of ``in_hw``, its launch configurations from the tuned table."""
    from .engine.tune import autotune_program
    if model_type == "multi_classifier":
        from .engine.inception import InceptionProgram
        prog = InceptionProgram(model, batch, device, in_hw=in_hw, p_drop=0.0)
    else:
        from .engine.mtl import MTLProgram
        prog = MTLProgram(model, batch, device, in_hw=in_hw)
    autotune_program(prog, measure=False)
    return prog


def window_runner(model: nn.Module, model_type: str, batch: int, device):
    """The lowered eval program of ``model`` and its step runner for resident-recording inference
    (:func:`resident_probs`); one runner serves any number of recordings."""
    from .engine.step import StepRunner
    return StepRunner(_eval_program(model, model_type, batch, device, WINDOW), None, None, use_graph=True)


def resident_probs(runner, rec: torch.Tensor, fs: np.ndarray, ts: np.ndarray, lo: int = 0,
                   hi: Optional[int] = None, gate=None):
    """Probabilities [N, K] (the tasks side by side) of windows ``[lo, hi)`` of the recording ``rec`` [C, F, T];
    the other rows are zero.  The recording is uploaded once; every batch is one replay of the runner's inference
    graph, with no host copy between the replays.  A recording of the shape, window starts and range of the
    runner's last one reuses its device buffers and its captured graph.

    ``gate`` = (gate_db, noise_floor) (:func:`predict_recording`): returns ``(table, active, power)``.  On the
    device: the power of all N windows, the floor, the ordered selection of the active windows of ``[lo, hi)``;
    their number is read back once (8 bytes) and the graph -- whose rows are numbered by the selection, the count
    read on the device -- is replayed ceil(count / B) times.  The rows of quiet windows stay zero; ``active`` is
    uint8 [N] over all windows, whatever the range."""
    from .ops import functional as HF
    prog = runner.p
    dev = prog.device
    n = len(fs) * len(ts)
    hi = n if hi is None else hi
    key = (tuple(rec.shape), tuple(int(v) for v in fs), tuple(int(v) for v in ts)) + (("gated",) if gate else ())
    src = runner.inference.get("infer")
    if src is not None and src.key == key:
        rec_d, fs_d, ts_d, table = (src.tensors[k] for k in ("rec", "fs", "ts", "probs"))
        sel, count = src.tensors.get("sel"), src.tensors.get("count")
        rec_d.copy_(rec)
        table.zero_()
    else:
        runner.clear_window_source()  # the last recording leaves before this one arrives
        rec_d = rec.to(device=dev, dtype=torch.float32, copy=True).contiguous()  # the runner's own buffer
        fs_d, ts_d = HF._starts(fs, dev), HF._starts(ts, dev)
        table = torch.zeros(n, sum(prog.prob_classes()), device=dev)
        sel = count = None
        if gate is not None:
            sel = torch.empty(n, dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
    if gate is None:
        runner.set_window_source(rec_d, fs_d, ts_d, table, lo, hi, key=key)
        for _ in range((hi - lo + prog.B - 1) // prog.B):
            runner.infer_step()
        return table.clone()
    gate_db, noise_floor = gate
    nf, nt = len(fs), len(ts)
    power = HF.window_power(rec_d, fs_d, ts_d, WINDOW)
    if _auto_floor(noise_floor):
        floor = torch.sort(power.view(nf, nt), 1).values[:, (nt - 1) // 2].contiguous()
    else:
        floor = torch.full((nf,), float(noise_floor), dtype=torch.float32, device=dev)
    _, _, active = HF.select_windows(power, floor, gate_db, nt, lo, hi, sel=sel, count=count)
    if (lo, hi) != (0, n):  # a shard: the selection is this range's, the flags are every window's on every rank
        active = HF.select_windows(power, floor, gate_db, nt, 0, n)[2]
    runner.set_window_source(rec_d, fs_d, ts_d, table, lo, hi, key=key, sel=sel, count=count)
    m = int(count.item())  # the one read-back
    for _ in range((m + prog.B - 1) // prog.B):
        runner.infer_step()
    return table.clone(), active, power


def _resident_probs(model: nn.Module, model_type: str, rec: torch.Tensor, fs, ts, lo: int, hi: int, batch: int,
                    device, gate=None):
    runner = window_runner(model, model_type, batch, device)
    try:
        return resident_probs(runner, rec, fs, ts, lo, hi, gate=gate)
    finally:
        runner.close()


def window_map_reference(probs: np.ndarray, fs, ts, shape: Tuple[int, int], cell: Tuple[int, int],
                         window: Tuple[int, int] = WINDOW) -> np.ndarray:
    """fp64 cell map [K, nfc, ntc] of per-window probabilities [N, K] (window ``n = a * len(ts) + b``): every
    sample's value is the mean of the windows that cover it, every cell's value the mean of its samples.  The
    windows covering sample (f, t) are (those covering row f) x (those covering time t), so

        map[k, i, j] = sum_a sum_b wf[a, i] wt[b, j] probs[a nt + b, k]

    with the per-axis weights of ``ops.functional.window_cell_weights``."""
    from .ops.functional import window_cell_weights
    wf = window_cell_weights(fs, window[0], shape[0], cell[0])
    wt = window_cell_weights(ts, window[1], shape[1], cell[1])
    p = np.asarray(probs, dtype=np.float64).reshape(len(fs), len(ts), -1)
    return np.einsum("ai,bj,abk->kij", wf, wt, p)


def prediction_map(res_or_probs, fs, ts, shape: Tuple[int, int], cell: Tuple[int, int],
                   window: Tuple[int, int] = WINDOW, active=None) -> Dict:
    """What an operator reads: cells of ``cell`` = (cf, ct) samples along the fiber and time of a recording of
    ``shape`` = (F, T).  A sample's probability is the mean over the windows that cover it, a cell's the mean over
    its samples.

    ``res_or_probs``: the dict :func:`predict_recording` returns, or a probability table [N, K] (K = 18: distance
    and event side by side, 16, 2, or Model C's 32 joint classes, marginalised by ``decode_joint``'s coding
    ``joint = distance + 16 * event``) as an array or a tensor.  A tensor on the GPU is aggregated there (HIP),
    anything else in numpy fp64.  Returns ``event_map`` [2, nfc, ntc], ``distance_map`` [16, nfc, ntc] and
    ``distance_mean_m`` [nfc, ntc] (1 class = 1 m), as far as the model has the task.

    ``active``: the flags [N] of a gated :func:`predict_recording` (taken from a result dict that has them).  Only
    active windows speak: the result gains ``activity_map`` [nfc, ntc], the window-weighted mean of the flags, and
    every class map is ``sum w p / sum w active`` over the active windows covering the cell -- NaN where the activity
    is 0, a cell nothing was said about.  The flag column rides along as class K + 1 of one map computation (on the
    device: one ``window_map`` launch); the division runs after it."""
    if isinstance(res_or_probs, dict):
        r = res_or_probs
        if "joint_prob" in r:
            table = r["joint_prob"]
        else:
            table = np.concatenate([r[k] for k in ("distance_prob", "event_prob") if k in r], 1)
        if active is None:
            active = r.get("active")
    else:
        table = res_or_probs
    on_device = isinstance(table, torch.Tensor) and table.is_cuda
    if active is not None:
        if on_device:
            flag = torch.as_tensor(active).to(table.device).reshape(-1, 1).float()
            table = torch.cat([table.float() * flag, flag], 1)
        else:
            table = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
            flag = (active.detach().cpu().numpy() if isinstance(active, torch.Tensor) else np.asarray(active))
            flag = flag.reshape(-1, 1).astype(np.float64)
            table = np.concatenate([table.astype(np.float64) * flag, flag], 1)
    if on_device:
        from .ops import functional as HF
        m = HF.window_map(table.float().contiguous(), fs, ts, shape, window, cell)
        if active is not None:
            m = _divide_by_activity(m)
        m = m.cpu().numpy().astype(np.float64)
    else:
        table = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table
        m = window_map_reference(table, fs, ts, shape, cell, window)
        if active is not None:
            m = _divide_by_activity(m)
    if active is None:
        return _task_maps(m)
    return dict(_task_maps(m[:-1]), activity_map=m[-1])


def _divide_by_activity(m):
    """A map [K + 1, ..] whose last class is the flag column's (``sum w active``), a tensor or an array, in place:
    the other classes become ``sum w p / sum w active``, NaN where the activity is 0."""
    if isinstance(m, torch.Tensor):
        m[:-1] = torch.where(m[-1] > 0, m[:-1] / m[-1], torch.full_like(m[:-1], float("nan")))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            m[:-1] = np.where(m[-1] > 0, m[:-1] / m[-1], np.nan)
    return m


def _task_maps(m: np.ndarray) -> Dict:
    """The event / distance maps of a class map [K, nfc, ntc] (K as :func:`prediction_map` lists them)."""
    K = m.shape[0]
    out = {}
    if K == 32:  # joint = distance + 16 * event
        j = m.reshape(2, 16, *m.shape[1:])
        out["event_map"], out["distance_map"] = j.sum(1), j.sum(0)
    elif K == 18:
        out["distance_map"], out["event_map"] = m[:16], m[16:]
    elif K == 16:
        out["distance_map"] = m
    elif K == 2:
        out["event_map"] = m
    else:
        raise ValueError(f"a probability table of {K} classes is none of the models'")
    if "distance_map" in out:
        d = np.arange(16, dtype=out["distance_map"].dtype)
        out["distance_mean_m"] = np.tensordot(d, out["distance_map"], 1)
    return out


# ---- live inference on a growing recording -----------------------------------------------------------------------
# The recording arrives as chunks [C, F, n] in time order.  Its time axis lives in a ring of R >= Wt + 1 columns
# (sample t at column t mod R); time index j = 0, 1, ... starts at j * st and window (j, a) has the number
# n = j * nf + a -- time-major, so new windows append at the end -- and is evaluated once j * st + Wt <= total.
# flush() ends the stream at T = total and adds the end-aligned index of window_starts if (T - Wt) mod st != 0.
# Cell column q of the map is final once (q + 1) * ct <= total - Wt: every regular window covering it has run, and
# the end-aligned window of any possible end starts at or after total - Wt.


def live_time_weights(q: int, ct: int, Wt: int, st: int, T: Optional[int] = None) -> Tuple[int, np.ndarray]:
    """``(jlo, w)``: the time indices ``jlo .. jlo + len(w) - 1`` that cover cell column ``q`` and their fp64 weights
    (:func:`ops.functional.window_cell_weights` of the time axis at that column, without the whole table).  ``T``
    None: the stream is still running and the column is final, so only regular indices cover it; otherwise the
    stream ended at ``T`` and the end-aligned index, if there is one, is the last regular index + 1."""
    c0 = q * ct
    c1 = c0 + ct if T is None else min(c0 + ct, T)
    if c1 <= c0:
        raise ValueError(f"cell column {q} is outside the recording")
    t = np.arange(c0, c1, dtype=np.int64)
    jl = np.maximum(0, -((Wt - 1 - t) // st))  # first regular index with j * st + Wt > t
    jh = t // st                               # last regular index with j * st <= t
    last = int(jh.max())
    end = np.zeros(len(t), dtype=bool)
    if T is not None:
        if T < Wt:
            raise ValueError(f"recording dimension {T} is shorter than the window {Wt}")
        nreg = (T - Wt) // st + 1
        jh = np.minimum(jh, nreg - 1)
        last = int(jh.max())
        if (T - Wt) % st != 0 and c1 > T - Wt:
            end = t >= T - Wt
            last = nreg
    cover = jh - jl + 1 + end
    if (cover <= 0).any():
        raise ValueError("the window starts do not cover the recording")
    inv = 1.0 / cover
    jlo = int(jl.min())
    w = np.zeros(last - jlo + 1)
    for j in range(jlo, last + 1):
        sel = end if (end.any() and j == last) else (jl <= j) & (j <= jh)
        w[j - jlo] = inv[sel].sum() / (c1 - c0)
    return jlo, w


class LiveBook:
    """The host's integer arithmetic of a live recording: how many time indices can be evaluated and how many cell
    columns are final at a given total, how ``push`` splits a chunk, and how many rows of the ring table are alive.
    It mirrors the device's scalars (csrc/live.hip ring_advance_kernel) and never reads them."""

    def __init__(self, Wt: int, st: int, ring: int, ct: Optional[int] = None, table_indices: Optional[int] = None,
                 history: Optional[int] = None):
        """``history``: a gated recording's noise floor reads the powers of the last ``history`` time indices (the
        power ring has the table's ``jcap`` indices): those count as needed too.  None: no gate."""
        if ring < Wt + 1:
            raise ValueError(f"a ring of {ring} time columns is below the window's {Wt} + 1")
        if st < 1 or (ct is not None and ct < 1):
            raise ValueError("stride and cell must be positive")
        self.Wt, self.st, self.R, self.ct = int(Wt), int(st), int(ring), ct
        # a sub-chunk adds at most (R - Wt) // st + 1 indices; a non-final column reaches back (Wt + ct) // st + 2
        carried = (self.Wt + ct) // self.st + 2 if ct is not None else 0
        if history is not None and history < 1:
            raise ValueError("the floor's history must be positive")
        self.history = None if history is None else int(history)
        carried = max(carried, self.history - 1 if self.history else 0)
        self.jcap = int(table_indices) if table_indices is not None else (self.R - self.Wt) // self.st + 1 + carried
        if self.jcap < 1:
            raise ValueError("the table needs at least one time index")
        self.total = 0     # time samples received
        self.j_done = 0    # time indices evaluated
        self.q_done = 0    # cell columns emitted
        self.jend = None   # (number, start) of the end-aligned index, once flushed
        self.flushed = False

    def indices(self, total: int) -> int:
        return (total - self.Wt) // self.st + 1 if total >= self.Wt else 0

    def final_columns(self, total: int) -> int:
        return (total - self.Wt) // self.ct if (self.ct is not None and total >= self.Wt) else 0

    def first_needed(self) -> int:
        """The oldest time index whose rows are still read: the table's by a column not yet emitted, the power
        ring's by the floor of the next index (``history - 1`` indices back)."""
        first = self.j_done
        if self.history:  # not clamped at 0: the floor launch asks for history - 1 + the new indices from the start
            first = self.j_done - (self.history - 1)
        if self.ct is not None:
            first = min(first, max(0, (self.q_done * self.ct - self.Wt) // self.st + 1))
        return first

    def split(self, n: int):
        """The sizes ``push`` appends a chunk of ``n`` samples in: at most R - Wt each, so the data of the oldest
        window not yet evaluated (it starts after total - Wt) survives the append."""
        step = self.R - self.Wt
        return [min(step, n - i) for i in range(0, n, step)]

    def time_start(self, j: int) -> int:
        return self.jend[1] if (self.jend is not None and j == self.jend[0]) else j * self.st

    def _check_table(self, j1: int, oldest: int):
        if j1 - oldest > self.jcap:
            raise ValueError(f"the probability table holds {self.jcap} time indices, this push needs {j1 - oldest} "
                             "(its own, those that non-final map columns still read and those of the noise floor's "
                             "history): a smaller chunk, a larger ring or table_indices")

    def check_push(self, n: int):
        """Raise before anything is written if a step of this push would overwrite live rows of the table."""
        self.check_steps(self.split(n))

    def check_steps(self, steps):
        """:meth:`check_push` for appends of ``steps`` samples in turn (a decimated push appends what each raw piece
        yields)."""
        if self.flushed:
            raise RuntimeError("push after flush")
        total, j_done, q_done = self.total, self.j_done, self.q_done
        try:
            for m in steps:
                self.advance(m)
        finally:
            self.total, self.j_done, self.q_done = total, j_done, q_done

    def advance(self, n: int):
        """Append ``n <= R - Wt`` samples: returns the time indices ``[j0, j1)`` to evaluate and the cell columns
        ``[q0, q1)`` that become final."""
        if self.flushed:
            raise RuntimeError("push after flush")
        if not 1 <= n <= self.R - self.Wt:
            raise ValueError(f"an append of {n} samples; 1 .. R - Wt = {self.R - self.Wt}")
        total = self.total + n
        j0, j1 = self.j_done, self.indices(total)
        self._check_table(j1, self.first_needed())
        q0, q1 = self.q_done, max(self.q_done, self.final_columns(total))
        self.total, self.j_done, self.q_done = total, j1, q1
        return (j0, j1), (q0, q1)

    def finish(self):
        """End the stream at T = total: the end-aligned index (if any) and every remaining column."""
        if self.flushed:
            raise RuntimeError("flush after flush")
        T = self.total
        j0 = j1 = self.j_done
        q0 = q1 = self.q_done
        if T >= self.Wt:
            if (T - self.Wt) % self.st != 0:
                j1 = j0 + 1
                self._check_table(j1, self.first_needed())
                self.jend = (j0, T - self.Wt)
            if self.ct is not None:
                q1 = -(-T // self.ct)
        self.flushed = True
        self.j_done, self.q_done = j1, q1
        return (j0, j1), (q0, q1)


def _task_names(model, model_type: str):
    names = {"MTL": ["distance", "event"], "single_distance": ["distance"], "single_event": ["event"],
             "multi_classifier": ["joint"]}[model_type]
    ncls = {"distance": 16, "event": 2, "joint": model.num_classes if model_type == "multi_classifier" else 0}
    return names, [ncls[t] for t in names]


def _live_gate(gate_db, noise_floor, history, warmup) -> Dict:
    """The checked gate of a :class:`LiveRecording`: ``floor`` None is the running floor, a number the fixed one
    (which has no history and no warm-up)."""
    from .ops.functional import MAX_FLOOR_HISTORY
    if isinstance(noise_floor, str):
        if noise_floor != "running":
            raise ValueError(f"noise_floor must be \"running\" or a power, got {noise_floor!r}: \"auto\" is the median "
                             "over a whole recording, and a stream has no end")
        history, warmup = int(history), int(warmup)
        if not 1 <= warmup <= history <= MAX_FLOOR_HISTORY:
            raise ValueError(f"1 <= floor_warmup <= floor_history <= {MAX_FLOOR_HISTORY}, got floor_warmup {warmup}, "
                             f"floor_history {history}")
        return {"gate_db": float(gate_db), "floor": None, "history": history, "warmup": warmup}
    return {"gate_db": float(gate_db), "floor": float(noise_floor), "history": 1, "warmup": 1}


class _TorchLive:
    """The torch backend of :class:`LiveRecording`: a host (or ``device``) ring and table, the module in fp32."""

    def __init__(self, model, model_type, C, F, R, fs, window, st, jcap, K, batch, device, gate=None):
        self.model, self.model_type, self.batch, self.device = model.eval().to(device), model_type, batch, device
        self.fs, self.window, self.st, self.jcap, self.R = fs, window, st, jcap, R
        self.ring = torch.full((C, F, R), float("nan"))
        # gated: one more column, 1 for an evaluated window (the rows of quiet windows are zero)
        self.gate, self.K = gate, K
        self.table = np.full((jcap * len(fs), K + (gate is not None)), np.nan, dtype=np.float32)
        self.recent = np.zeros((0, len(fs)))  # fp64 powers of the last history - 1 time indices
        self.total = 0

    common_mode = None  # "median" / "mean": removed from every chunk before it enters the ring

    def set_common_mode(self, how: str):
        self.common_mode = how

    def append(self, chunk: torch.Tensor):
        n = chunk.shape[2]
        cols = (self.total + torch.arange(n)) % self.R
        chunk = chunk.detach().to("cpu", torch.float32)
        if self.common_mode is not None:
            from .data.common_mode import common_mode_reference
            chunk = torch.from_numpy(common_mode_reference(chunk.numpy(), self.common_mode)[0])
        self.ring[:, :, cols] = chunk
        self.total += n

    def flush(self):
        pass

    def set_decimation(self, taps: np.ndarray, D: int, raw_step: int):
        from .data.resample import HostDecimator
        self.decimator = HostDecimator(taps, D)  # carries the raw samples on the host, in fp64

    def append_raw(self, piece: torch.Tensor, m: int, carry_len: int, skip: int):
        """A raw piece through the fp64 reference; the ``m`` outputs it completes, rounded to fp32, are appended."""
        y = self.decimator.push(piece.detach().cpu().numpy())
        if y.shape[-1] != m:
            raise AssertionError("the decimator and the recording's book disagree")
        if m:
            self.append(torch.from_numpy(y.astype(np.float32)))

    def _flags(self, starts):
        """The gate of the new windows by the fp64 references: (active, power, floor), each [m * nf] in number
        order.  Powers from :func:`window_power_reference` on the ring's columns, floors from
        :func:`running_floor_reference` over the carried powers and the new ones."""
        nf, Wt = len(self.fs), self.window[1]
        power = np.stack([window_power_reference(self.ring[:, :, (t0 + torch.arange(Wt)) % self.R], self.fs, [0],
                                                 self.window) for _, t0 in starts])
        g = self.gate
        if g["floor"] is None:
            k = len(self.recent)  # min(j0, history - 1) rows: the reference's rows from k on are the whole stream's
            tail = np.concatenate([self.recent, power])
            floor = running_floor_reference(tail.reshape(-1), nf, g["history"], g["warmup"])[k:]
            self.recent = tail[max(0, len(tail) - (g["history"] - 1)):] if g["history"] > 1 else self.recent
        else:
            floor = np.full(power.shape, float(g["floor"]))
        return live_active_reference(power, floor, g["gate_db"]).reshape(-1), power.reshape(-1), floor.reshape(-1)

    def evaluate(self, starts):
        """``starts``: [(j, t0)].  Evaluates the windows (j, a) in number order; returns their rows [m * nf, K] and
        None -- gated: only the active ones go through the module, the rows are [m * nf, K + 1] (quiet: zero) and
        come with the flags ``(active, power, floor)``."""
        nf, (Wf, Wt) = len(self.fs), self.window
        if not starts:
            return np.zeros((0, self.table.shape[1]), dtype=np.float32), None
        flags = self._flags(starts) if self.gate is not None else None
        tiles = []
        for k, (j, t0) in enumerate(starts):
            cols = (t0 + torch.arange(Wt)) % self.R
            for a, f0 in enumerate(self.fs):
                if flags is None or flags[0][k * nf + a]:
                    tiles.append(self.ring[:, int(f0):int(f0) + Wf][:, :, cols])
        rows = []
        for i in range(0, len(tiles), self.batch):
            ps = _torch_probs(self.model, self.model_type, torch.stack(tiles[i:i + self.batch]).to(self.device))
            rows.append(torch.cat([p.float() for p in ps], 1).cpu())
        rows = torch.cat(rows).numpy() if rows else np.zeros((0, self.K), dtype=np.float32)
        if flags is not None:
            full = np.zeros((len(starts) * nf, self.K + 1), dtype=np.float32)
            full[flags[0], :self.K] = rows
            full[flags[0], self.K] = 1.0
            rows = full
        for k, (j, _) in enumerate(starts):
            r = (j % self.jcap) * nf
            self.table[r:r + nf] = rows[k * nf:(k + 1) * nf]
        return rows, flags

    def map_columns(self, wf: np.ndarray, cols) -> np.ndarray:
        """fp64 [K, nfc, ncol]; ``wf``: fp64 [nf, nfc]; ``cols``: [(jlo, w)] per column.  Gated: [K + 1, ..], the
        flag column's map last and the classes divided by it."""
        nf = len(self.fs)
        out = np.zeros((self.table.shape[1], wf.shape[1], len(cols)))
        for q, (jlo, w) in enumerate(cols):
            rows = [(j % self.jcap) * nf for j in range(jlo, jlo + len(w))]
            p = np.stack([self.table[r:r + nf] for r in rows]).astype(np.float64)  # [jn, nf, K]
            out[:, :, q] = np.einsum("ai,j,jak->ki", wf, w, p)
        return _divide_by_activity(out) if self.gate is not None else out

    def close(self):
        pass


class _EngineLive:
    """The engine backend: device ring, device scalars and ring table; one captured graph per live source.  Gated
    (csrc/live_gate.hip): rings of the windows' powers, floors and flags beside the table, which gains the
    "evaluated" column; the graph's rows are numbered by the selection of the piece just appended."""

    def __init__(self, model, model_type, C, F, R, fs, window, st, jcap, K, batch, device, gate=None):
        from .ops import functional as HF
        if window != WINDOW:
            raise ValueError(f"the lowered models take {WINDOW} windows")
        self.HF, self.fs, self.window, self.st, self.jcap, self.R = HF, fs, window, st, jcap, R
        self.runner = window_runner(model, model_type, batch, device)
        self.B = self.runner.p.B
        dev = self.runner.p.device
        self.ring = torch.zeros(C, F, R, device=dev)
        self.state = HF.live_state(dev)
        self.gate, self.K = gate, K
        self.table = torch.zeros(jcap * len(fs), K + (gate is not None), device=dev)
        self.fs_d = HF._starts(fs, dev)
        by = {}
        if gate is not None:
            n = jcap * len(fs)
            self.power = torch.full((n,), float("nan"), device=dev)
            # a fixed floor fills its ring once and running_floor is never launched
            self.floor = torch.full((n,), float(gate["floor"]) if gate["floor"] is not None else 0.0, device=dev)
            self.active = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.sel = torch.full((n,), -1, dtype=torch.int64, device=dev)  # a piece adds at most jcap indices
            self.cursor, self.count = HF.live_gate_state(dev)
            by = {"sel": self.sel, "count": self.count, "cursor": self.cursor}
        # one pinned staging buffer and its device twin, reused by every push
        self.stage_h = torch.empty(C * F * (R - window[1]), dtype=torch.float32).pin_memory()
        self.stage_d = torch.empty(C * F * (R - window[1]), dtype=torch.float32, device=dev)
        self.staged = None  # event: the last upload from stage_h has finished
        self.runner.set_live_source(self.ring, self.fs_d, self.state, self.table, st, jcap, **by)
        self.runner.prepare_live()  # the one capture

    def append(self, chunk: torch.Tensor):
        C, Fn, n = chunk.shape
        dst = self.stage_d[:C * Fn * n].view(C, Fn, n)
        if chunk.is_cuda:
            dst.copy_(chunk)
        else:
            if self.staged is not None:
                self.staged.synchronize()  # the buffer is being read until then
            src = self.stage_h[:C * Fn * n].view(C, Fn, n)
            src.copy_(chunk)
            dst.copy_(src, non_blocking=True)
            self.staged = torch.cuda.Event()
            self.staged.record()
        self._clean(dst)
        self.HF.ring_append(self.ring, self.state, dst, len(self.fs), self.st, self.window[1])

    common_mode = None  # "median" / "mean": removed from every staged chunk before it enters the ring

    def set_common_mode(self, how: str):
        """The common-mode stage: one eager launch, in place, on the staged chunk ahead of each ``ring_append`` --
        outside the captured graph, and nothing is read back.  ``cm_trace`` takes the values subtracted (the
        launch's own buffer; the live path does not return them)."""
        self.common_mode = how
        self.cm_trace = torch.empty(self.ring.shape[0] * (self.R - self.window[1]), device=self.ring.device)

    def _clean(self, dst: torch.Tensor):
        if self.common_mode is not None:
            C, _, n = dst.shape
            self.HF.common_mode(dst, self.common_mode, out=dst, trace=self.cm_trace[:C * n].view(C, n))

    def flush(self):
        self.HF.ring_append(self.ring, self.state, None, len(self.fs), self.st, self.window[1], flush=True)

    def set_decimation(self, taps: np.ndarray, D: int, raw_step: int):
        """The raw front end: the taps, the two carry buffers a launch reads and writes in turn, and one pinned raw
        staging buffer with its device twin for pieces of at most ``raw_step`` raw samples per row (bytes: an fp32
        or an int16 piece is staged as it is)."""
        C, Fn, _ = self.ring.shape
        dev = self.ring.device
        self.D, self.taps_d = D, torch.from_numpy(taps).to(dev)
        self.carry, self.cur = self.HF.decimate_carry(C * Fn, len(taps), dev), 0
        self.raw_h = torch.empty(4 * C * Fn * raw_step, dtype=torch.uint8).pin_memory()
        self.raw_d = torch.empty(4 * C * Fn * raw_step, dtype=torch.uint8, device=dev)
        self.raw_staged = None  # event: the last upload from raw_h has finished

    def append_raw(self, piece: torch.Tensor, m: int, carry_len: int, skip: int):
        """A raw piece [C, F, n] (fp32 or int16) -> fir_decimate -> the decimated staging buffer -> ring_append.  A
        piece on the device is read where it is; one on the host goes through the raw staging buffers."""
        C, Fn, n = piece.shape
        if piece.is_cuda:
            raw = piece
        else:
            if self.raw_staged is not None:
                self.raw_staged.synchronize()  # the buffer is being read until then
            cnt = C * Fn * n
            src = self.raw_h.view(piece.dtype)[:cnt].view(C, Fn, n)
            src.copy_(piece)
            raw = self.raw_d.view(piece.dtype)[:cnt].view(C, Fn, n)
            raw.copy_(src, non_blocking=True)
            self.raw_staged = torch.cuda.Event()
            self.raw_staged.record()
        dst = self.stage_d[:C * Fn * m].view(C, Fn, m)
        self.HF.fir_decimate(raw, self.carry[self.cur], carry_len, skip, self.taps_d, self.D, out=dst, m=m,
                             carry_out=self.carry[1 - self.cur])
        self.cur = 1 - self.cur
        if m:
            self._clean(dst)
            self.HF.ring_append(self.ring, self.state, dst, len(self.fs), self.st, self.window[1])

    def evaluate(self, starts):
        """As :meth:`_TorchLive.evaluate`.  Gated: power, floor and selection of the new windows are launched eagerly
        (the range is the host's, LiveBook's), the count is read once (8 bytes) and the graph replayed
        ceil(count / B) times."""
        nf, HF = len(self.fs), self.HF
        m = len(starts) * nf
        if m == 0:
            return np.zeros((0, self.table.shape[1]), dtype=np.float32), None
        if self.gate is not None:
            g, (n0, n1) = self.gate, (starts[0][0] * nf, (starts[-1][0] + 1) * nf)
            HF.ring_window_power(self.ring, self.state, self.fs_d, self.st, self.window, self.power, self.jcap, n0, n1)
            if g["floor"] is None:
                HF.running_floor(self.power, self.floor, nf, self.jcap, n0, n1, g["history"], g["warmup"])
            HF.live_select(self.power, self.floor, self.active, self.table, self.state, self.sel, self.count,
                           self.cursor, g["gate_db"], nf, self.jcap, n0, n1)
            m = int(self.count.item())  # the one read-back
        for _ in range((m + self.B - 1) // self.B):
            self.runner.live_step()
        rows = torch.as_tensor([(j % self.jcap) * nf + a for j, _ in starts for a in range(nf)],
                               dtype=torch.int64).to(self.table.device)
        flags = None
        if self.gate is not None:
            flags = tuple(t.index_select(0, rows).cpu().numpy() for t in (self.active, self.power, self.floor))
            flags = (flags[0].astype(bool),) + flags[1:]
        return self.table.index_select(0, rows).cpu().numpy(), flags

    def map_columns(self, wf, cols) -> np.ndarray:
        F_ = self.ring.shape[1]
        m = self.HF.live_map(self.table, self.fs, F_, self.window[0], self.cf, self.jcap, [c[0] for c in cols],
                             [c[1] for c in cols])
        if self.gate is not None:  # the flag column rode along as class K + 1: the division runs after the launch
            m = _divide_by_activity(m)
        return m.cpu().numpy().astype(np.float64)

    def close(self):
        if self.runner is not None:
            self.runner.clear_live_source()
            self.runner.close()
            self.runner = None


class LiveRecording:
    """Sliding-window inference on a recording that is still growing.

    ``push(chunk)`` takes the next ``[C, F, n]`` (or ``[F, n]``) time samples, on the CPU or the device, and returns
    the predictions of the windows that became available -- ``positions`` [m, 2] and per task ``<task>_pred`` /
    ``<task>_prob``, as :func:`predict_recording` -- in evaluation order (time-major).  With ``cell`` = (cf, ct) it
    also returns ``map_columns``: ``first`` / ``last`` (one past) of the cell columns that became final and their
    ``event_map`` / ``distance_map`` / ``distance_mean_m`` slices [.., nfc, last - first] (and ``class_map``, every
    class of the probability table before the tasks are marginalised); a column is returned once
    and never revised.  ``flush()`` ends the stream: the end-aligned window of :func:`window_starts` and every
    remaining column.  Over all calls the windows are exactly those of ``predict_recording(rec, stride=stride)`` on
    the concatenated chunks, and the columns those of :func:`prediction_map`.

    ``ring``: time columns kept (>= window + 1); a chunk longer than ``ring - window`` is appended in pieces.
    ``table_indices``: time indices the probability table holds (default: enough for any push); a push that would
    overwrite rows still needed raises before it changes anything.  On the engine backend the ring, the window
    counters and the table live on the device and every batch is one replay of one graph captured at construction
    (``captures`` stays at 1); the torch backend keeps a host ring and evaluates the module in fp32.

    ``gate_db``: the activity gate of :func:`predict_recording` on the growing recording -- a window is active unless
    its power is below its noise floor times ``10^(gate_db / 10)``, and only active windows are evaluated.
    ``noise_floor``: a power (one floor everywhere), or ``"running"``: per fiber start the lower median of the powers
    of the last ``floor_history`` time indices, the window's own included (:func:`running_floor_reference`; causal, no
    look-ahead), and no floor -- every window active -- before ``floor_warmup`` of them exist.  (``"auto"``, the
    median over the whole recording, needs the stream's end and is refused.)  A trailing median follows a level that
    persists: an event longer than about ``floor_history / 2`` time indices becomes the floor and fades from the
    flags; a floor that freezes while windows are active would depend on its own flags and is not offered.  The
    results gain ``active`` [m] bool, ``power_db`` [m] and ``floor_db`` [m] (-inf while warming up); a quiet window
    has ``<task>_pred`` -1 and a zero ``<task>_prob`` row, and ``map_columns`` gains ``activity_map``
    [nfc, ncols], its class maps being ``sum w p / sum w active`` (NaN where the activity is 0) as
    ``prediction_map(active=...)``; ``class_map`` is that divided map.  With a fixed floor the calls together equal
    ``predict_recording(rec, gate_db=..., noise_floor=P)`` and its map on the concatenated chunks.  On the engine
    backend power, floor and the ordered selection of each appended piece run on the device (csrc/live_gate.hip), the
    count of active windows is read back once per piece and the one graph replayed ceil(count / batch) times.  None:
    no gate, every window evaluated.

    ``decimate`` = D: ``push`` takes **raw** chunks ``[C, F, n_raw]`` (fp32 or int16, host or device), which go
    through the FIR ``taps`` (None: ``data.resample.decimation_taps(D)``) and decimation by D ahead of the ring
    (:func:`decimate_recording` is the whole-recording form); ``stride``, ``cell``, ``ring``, ``table_indices``,
    ``floor_history`` and ``total`` stay in decimated samples, as the model sees them.  The chunk is processed in raw
    pieces that each yield at most ``ring - window`` outputs; the raw samples that the next output still needs (at
    most L - 1 per row) are carried across pieces and pushes, on the engine backend on the device
    (csrc/resample.hip; ``DecimatorBook`` mirrors the counts on the host), so the decimated stream -- and with it
    every result -- has the same bits however the raw stream is cut.  A push that completes no output returns an
    empty result; ``flush()`` drops the carried raw samples.  The results gain ``raw_time_start`` /
    ``raw_time_stop`` as :func:`predict_recording`'s.  None: chunks are at the model's rate.

    ``common_mode`` = ``"median"`` or ``"mean"``: the common mode (:func:`remove_common_mode`) is removed from every
    piece before it enters the ring -- with ``decimate`` from the decimated piece, as :func:`predict_recording`
    does.  Time columns are independent, so nothing is carried and the calls together equal
    ``predict_recording(rec, common_mode=...)`` on the concatenated chunks.  On the engine backend it is one eager
    launch, in place, on the staged chunk ahead of each append (csrc/common_mode.hip): outside the captured graph
    (``captures`` stays at 1), nothing read back, and a device chunk passed in is not modified.  The values
    subtracted are not returned by the live path.  None: nothing is removed."""

    RAW_PIECE = 1 << 24  # raw elements staged per piece at most (and never below one decimation's D per row)

    def __init__(self, model: nn.Module, model_type: str, F: int, C: int = 1, stride=(100, 125), cell=None,
                 ring: int = 8 * WINDOW[1], batch: int = 32, device=None, use_engine: Optional[bool] = None,
                 ctx: Optional[DistContext] = None, table_indices: Optional[int] = None, window=WINDOW,
                 gate_db: Optional[float] = None, noise_floor="running", floor_history: int = 64,
                 floor_warmup: int = 8, decimate: Optional[int] = None, taps=None,
                 common_mode: Optional[str] = None):
        if ctx is not None and ctx.enabled and ctx.world > 1:
            raise ValueError("a live recording is not sharded: world > 1 is not supported")
        self.decimate, self.taps = _decimation(decimate, taps)
        from .data.common_mode import as_common_mode
        self.common_mode = as_common_mode(common_mode)
        self.gate = None
        if gate_db is not None:
            self.gate = _live_gate(gate_db, noise_floor, floor_history, floor_warmup)
        device = torch.device(device) if device is not None else (ctx.device if ctx else torch.device("cpu"))
        if use_engine is None:
            use_engine = device.type == "cuda"
        self.model_type, self.F, self.C, self.window = model_type, int(F), int(C), tuple(window)
        self.stride = (int(stride[0]), int(stride[1]))
        self.cell = None if cell is None else (int(cell[0]), int(cell[1]))
        self.fs = window_starts(self.F, self.window[0], self.stride[0])
        self.book = LiveBook(self.window[1], self.stride[1], int(ring), None if cell is None else self.cell[1],
                             table_indices, history=None if self.gate is None else self.gate["history"])
        self.names, self.ncls = _task_names(model, model_type)
        K = sum(self.ncls)
        if self.cell is not None:
            from .ops.functional import window_cell_weights
            if min(self.cell) < 1 or self.stride[1] > self.window[1]:
                raise ValueError(f"a map needs a positive cell and windows that cover the recording: time stride "
                                 f"at most {self.window[1]}")
            self.wf = window_cell_weights(self.fs, self.window[0], self.F, self.cell[0])  # raises if rows uncovered
        backend = _EngineLive if use_engine else _TorchLive
        self.backend = backend(model, model_type, self.C, self.F, int(ring), self.fs, self.window, self.stride[1],
                               self.book.jcap, K, batch, device, **({} if self.gate is None else {"gate": self.gate}))
        self.backend.cf = self.cell[0] if self.cell is not None else None
        if self.common_mode is not None:
            self.backend.set_common_mode(self.common_mode)
        if self.decimate is not None:
            from .data.resample import DecimatorBook
            self.dbook = DecimatorBook(len(self.taps), self.decimate)
            # n raw samples complete at most (n - 1) // D + 1 outputs: a piece of (R - Wt) D fits one append
            per_row = max(self.decimate, self.RAW_PIECE // (self.C * self.F))
            self.raw_step = min((int(ring) - self.window[1]) * self.decimate, per_row)
            self.backend.set_decimation(self.taps, self.decimate, self.raw_step)

    @property
    def total(self) -> int:
        return self.book.total

    @property
    def captures(self) -> int:
        """Graph captures so far (engine backend; 0 on the torch backend)."""
        r = getattr(self.backend, "runner", None)
        return r.captures if r is not None else 0

    def _result(self, evals, starts, q_first: int, maps) -> Dict:
        """``evals``: per step the new windows' table rows and (gated) their flags; ``maps``: the class maps of the
        steps' new columns."""
        K, gated = sum(self.ncls), self.gate is not None
        pos = np.asarray([(int(f0), t0) for _, t0 in starts for f0 in self.fs], dtype=np.int64).reshape(-1, 2)
        rows = np.concatenate([e[0] for e in evals]) if evals else np.zeros((0, K + gated), dtype=np.float32)
        probs = [p.contiguous() for p in torch.from_numpy(rows[:, :K].copy()).split(self.ncls, 1)]
        flags = None
        if gated:
            got = [e[1] for e in evals if e[1] is not None]
            active, power, floor = (np.concatenate([g[i] for g in got]) if got else np.zeros(0, dtype=dt)
                                    for i, dt in enumerate((bool, np.float64, np.float64)))
            flags = (active, power)
        res = _result(self.model_type, self.names, probs, pos, None, flags)
        if self.decimate is not None:
            _raw_times(res, self.decimate, len(self.taps), self.window[1])
        if gated:
            res["floor_db"] = _power_db(floor)
        if self.cell is not None:
            maps = [m for m in maps if m is not None]
            nfc = -(-self.F // self.cell[0])
            m = np.concatenate(maps, 2) if maps else np.zeros((K + gated, nfc, 0))
            # class_map: every class of the table, before the tasks are marginalised (gated: divided by the activity)
            if gated:
                res["map_columns"] = dict(_task_maps(m[:-1]), first=q_first, last=self.book.q_done, class_map=m[:-1],
                                          activity_map=m[-1])
            else:
                res["map_columns"] = dict(_task_maps(m), first=q_first, last=self.book.q_done, class_map=m)
        return res

    def _emit(self, q0: int, q1: int, T: Optional[int]):
        """The class map [K, nfc, q1 - q0] of the columns that became final."""
        if q1 <= q0:
            return None
        cols = [live_time_weights(q, self.cell[1], self.window[1], self.stride[1], T) for q in range(q0, q1)]
        return self.backend.map_columns(self.wf, cols)

    @torch.no_grad()
    def push(self, chunk) -> Dict:
        if self.book.flushed:
            raise RuntimeError("push after flush")
        chunk = torch.as_tensor(chunk)
        if chunk.dim() == 2:
            chunk = chunk.unsqueeze(0)
        if chunk.dim() != 3 or chunk.shape[0] != self.C or chunk.shape[1] != self.F or chunk.shape[2] < 1:
            raise ValueError(f"a chunk must be [{self.C}, {self.F}, n >= 1], got {tuple(chunk.shape)}")
        if self.decimate is not None:
            return self._push_raw(chunk)
        n = chunk.shape[2]
        self.book.check_push(n)
        rows, starts, maps, q_first, at = [], [], [], self.book.q_done, 0
        for m in self.book.split(n):
            (j0, j1), (q0, q1) = self.book.advance(m)
            self.backend.append(chunk[:, :, at:at + m].float())
            at += m
            new = [(j, self.book.time_start(j)) for j in range(j0, j1)]
            rows.append(self.backend.evaluate(new))
            starts += new
            if self.cell is not None:
                maps.append(self._emit(q0, q1, None))
        return self._result(rows, starts, q_first, maps)

    def _push_raw(self, chunk: torch.Tensor) -> Dict:
        """``push`` of a raw chunk: raw pieces of at most ``raw_step`` samples, each decimated into the staging
        buffer and, if it completes outputs, appended and evaluated as a chunk of ``push`` is."""
        chunk = _raw_recording(chunk)
        if chunk.is_cuda and not chunk.is_contiguous():
            chunk = chunk.contiguous()
        n = chunk.shape[2]
        sizes = [min(self.raw_step, n - i) for i in range(0, n, self.raw_step)]
        plan = self.dbook.plan(sizes)
        outputs = sum(p[0] for p in plan)
        if outputs:  # before anything is written: the push as a whole, and as the appends it will make
            self.book.check_push(outputs)
            self.book.check_steps([p[0] for p in plan if p[0]])
        rows, starts, maps, q_first, at = [], [], [], self.book.q_done, 0
        for size in sizes:
            m, carry_len, skip = self.dbook.push(size)
            self.backend.append_raw(chunk[:, :, at:at + size], m, carry_len, skip)
            at += size
            if m == 0:
                continue
            (j0, j1), (q0, q1) = self.book.advance(m)
            new = [(j, self.book.time_start(j)) for j in range(j0, j1)]
            rows.append(self.backend.evaluate(new))
            starts += new
            if self.cell is not None:
                maps.append(self._emit(q0, q1, None))
        return self._result(rows, starts, q_first, maps)

    @torch.no_grad()
    def flush(self) -> Dict:
        q_first = self.book.q_done
        (j0, j1), (q0, q1) = self.book.finish()
        self.backend.flush()
        new = [(j, self.book.time_start(j)) for j in range(j0, j1)]
        rows = [self.backend.evaluate(new)]
        maps = [self._emit(q0, q1, self.book.total)] if self.cell is not None else []
        return self._result(rows, new, q_first, maps)

    def close(self):
        """Release the backend (the engine's graph, ring and table)."""
        if self.backend is not None:
            self.backend.close()
            self.backend = None

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


def _torch_probs(model: nn.Module, model_type: str, x: torch.Tensor) -> Sequence[torch.Tensor]:
    out = model(x)
    if model_type == "multi_classifier":
        return [torch.softmax(out[0] if isinstance(out, tuple) else out, 1)]
    outs = out if isinstance(out, tuple) else (out,)
    return [o.exp() for o in outs]  # A/B heads emit log-probabilities


@torch.no_grad()
def predict_recording(model: nn.Module, model_type: str, rec: torch.Tensor, stride=(100, 125), batch: int = 32,
                      ctx: Optional[DistContext] = None, device=None, use_engine: Optional[bool] = None,
                      windows: Optional[str] = None, runner=None) -> Dict:
    """Per-window predictions for one recording.  Returns numpy arrays: ``positions`` [N, 2], and per task
    (``distance`` / ``event`` as the model provides) ``<task>_pred`` [N] and ``<task>_prob`` [N, k].

    ``windows``: ``"resident"`` (the engine path's default) uploads the recording once and cuts the windows on
    the device; ``"materialize"`` (the torch backend's only form) builds the window stack on the host.
    ``runner``: a :func:`window_runner` of this model to reuse over many recordings (resident windows only; its
    batch size holds); without one the call lowers the model itself."""
    device = torch.device(device) if device is not None else (ctx.device if ctx else torch.device("cpu"))
    if use_engine is None:
        use_engine = device.type == "cuda"
    if windows is None:
        windows = "resident" if use_engine else "materialize"
    if windows not in ("resident", "materialize"):
        raise ValueError(f"windows must be 'resident' or 'materialize', got {windows!r}")
    if windows == "resident" and not use_engine:
        raise ValueError("windows='resident' needs the engine backend")
    if runner is not None and windows != "resident":
        raise ValueError("a window runner serves windows='resident' only")
    names = {"MTL": ["distance", "event"], "single_distance": ["distance"], "single_event": ["event"],
             "multi_classifier": ["joint"]}[model_type]
    ncls = {"distance": 16, "event": 2, "joint": model.num_classes if model_type == "multi_classifier" else 0}
    if windows == "resident":
        rec3 = rec.float().unsqueeze(0) if rec.dim() == 2 else rec.float()
        fs, ts = window_starts(rec3.shape[1], WINDOW[0], stride[0]), window_starts(rec3.shape[2], WINDOW[1], stride[1])
        pos = np.stack(np.meshgrid(fs, ts, indexing="ij"), -1).reshape(-1, 2)
        n = len(pos)
        lo, hi = _shard(n, ctx)
        if runner is not None:
            table = resident_probs(runner, rec3, fs, ts, lo, hi)
        else:
            table = _resident_probs(model, model_type, rec3, fs, ts, lo, hi, batch, device)
        probs = [p.contiguous() for p in table.split([ncls[t] for t in names], 1)]
        return _result(model_type, names, probs, pos, ctx)
    tiles, pos = sliding_windows(rec.float(), stride=stride)
    n = len(tiles)
    lo, hi = _shard(n, ctx)
    mine = tiles[lo:hi].to(device)
    probs = [torch.zeros(n, ncls[t], device=device) for t in names]
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
            probs[t][lo:hi] = chunks[t].float()
    return _result(model_type, names, probs, pos, ctx)


def _result(model_type: str, names, probs, pos, ctx: Optional[DistContext]) -> Dict:
    """The result dict from the per-task probability tables (each rank filled its own rows of a zeroed table)."""
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
    return res


def _engine_probs(model: nn.Module, model_type: str, x: torch.Tensor, batch: int, device) -> Sequence[torch.Tensor]:
    """Eval-mode forward of the lowered program over window batches (the last batch padded)."""
    from .engine.step import StepRunner
    n = len(x)
    if model_type == "multi_classifier":
        from .engine.inception import InceptionProgram
        prog = InceptionProgram(model, batch, device, in_hw=tuple(x.shape[2:]), p_drop=0.0)
        labels = torch.zeros(n, dtype=torch.int64, device=device)
    else:
        from .engine.mtl import MTLProgram
        prog = MTLProgram(model, batch, device, in_hw=tuple(x.shape[2:]))
        labels = torch.zeros(n, 2, dtype=torch.int64, device=device)
    from .engine.tune import autotune_program
    autotune_program(prog, measure=False)
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


def window_runner(model: nn.Module, model_type: str, batch: int, device):
    """The lowered eval program of ``model`` and its step runner for resident-recording inference
    (:func:`resident_probs`); one runner serves any number of recordings."""
    from .engine.step import StepRunner
    from .engine.tune import autotune_program
    if model_type == "multi_classifier":
        from .engine.inception import InceptionProgram
        prog = InceptionProgram(model, batch, device, in_hw=WINDOW, p_drop=0.0)
    else:
        from .engine.mtl import MTLProgram
        prog = MTLProgram(model, batch, device, in_hw=WINDOW)
    autotune_program(prog, measure=False)
    return StepRunner(prog, None, None, use_graph=True)


def resident_probs(runner, rec: torch.Tensor, fs: np.ndarray, ts: np.ndarray, lo: int = 0,
                   hi: Optional[int] = None) -> torch.Tensor:
    """Probabilities [N, K] (the tasks side by side) of windows ``[lo, hi)`` of the recording ``rec`` [C, F, T];
    the other rows are zero.  The recording is uploaded once; every batch is one replay of the runner's inference
    graph, with no host copy between the replays.  A recording of the shape, window starts and range of the
    runner's last one reuses its device buffers and its captured graph."""
    prog = runner.p
    dev = prog.device
    n = len(fs) * len(ts)
    hi = n if hi is None else hi
    key = (tuple(rec.shape), tuple(int(v) for v in fs), tuple(int(v) for v in ts))
    if runner.window is not None and runner.window_key == key:
        rec_d, fs_d, ts_d, table = runner.window[:4]
        rec_d.copy_(rec)
        table.zero_()
    else:
        runner.clear_window_source()  # the last recording leaves before this one arrives
        rec_d = rec.to(device=dev, dtype=torch.float32, copy=True).contiguous()  # the runner's own buffer
        fs_d = torch.as_tensor(np.asarray(fs), dtype=torch.int32).to(dev)
        ts_d = torch.as_tensor(np.asarray(ts), dtype=torch.int32).to(dev)
        table = torch.zeros(n, sum(prog.prob_classes()), device=dev)
    runner.set_window_source(rec_d, fs_d, ts_d, table, lo, hi, key=key)
    for _ in range((hi - lo + prog.B - 1) // prog.B):
        runner.infer_step()
    return table.clone()


def _resident_probs(model: nn.Module, model_type: str, rec: torch.Tensor, fs, ts, lo: int, hi: int, batch: int,
                    device) -> torch.Tensor:
    runner = window_runner(model, model_type, batch, device)
    try:
        return resident_probs(runner, rec, fs, ts, lo, hi)
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
                   window: Tuple[int, int] = WINDOW) -> Dict:
    """What an operator reads: cells of ``cell`` = (cf, ct) samples along the fiber and time of a recording of
    ``shape`` = (F, T).  A sample's probability is the mean over the windows that cover it, a cell's the mean over
    its samples.

    ``res_or_probs``: the dict :func:`predict_recording` returns, or a probability table [N, K] (K = 18: distance
    and event side by side, 16, 2, or Model C's 32 joint classes, marginalised by ``decode_joint``'s coding
    ``joint = distance + 16 * event``) as an array or a tensor.  A tensor on the GPU is aggregated there (HIP),
    anything else in numpy fp64.  Returns ``event_map`` [2, nfc, ntc], ``distance_map`` [16, nfc, ntc] and
    ``distance_mean_m`` [nfc, ntc] (1 class = 1 m), as far as the model has the task."""
    if isinstance(res_or_probs, dict):
        r = res_or_probs
        if "joint_prob" in r:
            table = r["joint_prob"]
        else:
            table = np.concatenate([r[k] for k in ("distance_prob", "event_prob") if k in r], 1)
    else:
        table = res_or_probs
    if isinstance(table, torch.Tensor) and table.is_cuda:
        from .ops import functional as HF
        m = HF.window_map(table.float().contiguous(), fs, ts, shape, window, cell).cpu().numpy().astype(np.float64)
    else:
        table = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table
        m = window_map_reference(table, fs, ts, shape, cell, window)
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

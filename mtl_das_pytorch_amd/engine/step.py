"""Train / eval step execution for a lowered program, with HIP-graph capture.

A training step is

    [gather batch + zero the arena's accumulators] [forward] [backward]  ->  (DP: RCCL all-reduce of the flat
    gradient buckets)  ->  [fused Adam + bf16 re-pack] [step++]

Single GPU: the whole step is ONE captured HIP graph (``torch.cuda.CUDAGraph`` is a hipGraph on ROCm),
so a step costs one graph launch from the host.  Data parallel with capturable collectives (a 1-rank RCCL
group, see DistContext.capturable_collectives): still ONE graph -- the gradient buckets' all-reduces are
captured on a communication stream inside it (LoweredProgram.backward_with_allreduce), each waiting only for
its bucket's finalize.  Otherwise (the multi-rank default: RCCL collectives stay eager) forward + backward
are ONE graph that records an EXTERNAL event where each gradient bucket is complete
(LoweredProgram.backward_with_ext_events); after enqueuing its replay the host makes the communication
stream wait for bucket k's event and issues bucket k's asynchronous RCCL all-reduce there, so it runs while
the graph computes the rest of the backward; the optimizer graph waits for every bucket (Work.wait).

The batch indices come from a device-resident schedule (set_index_schedule: the gather reads the next row,
the optimizer kernel advances the cursor) or from a persistent device buffer the host refreshes before each
replay; the learning rate is a device scalar, so the reference's LR schedule never forces a re-capture.

With SNR noise on (set_train_noise / set_eval_noise) the gather is the noise gather of csrc/augment.hip: the levels
and the draw number are device scalars too, a training gather phase ends with the launch that advances the draw, and
the power table of a bound set is computed once.

An inference step over a resident recording (set_window_source / infer_step) is

    [window gather from the recording] [eval forward] [probabilities -> resident table, batch cursor++]

one graph too: the batch's windows are numbered by a device cursor that the step's last kernel advances, so the
replays that cover a recording need no host copy between them.

A live step over a growing recording (set_live_source / live_step) is the same graph over a time ring:

    [ring gather of windows next .. next + B - 1] [eval forward] [probabilities -> ring table, next += valid rows]

The ring, the counters and the table are device state that ring_append and the graph advance, so one capture serves
every push of the stream; ``captures`` counts the captures of a runner.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ..data.noise import EVAL_SEED, parse_snr_range
from .program import EngineStreams, EventKeeper, ExtEvent, NoiseSpec, Phase


class StateSnapshot:
    """Save/restore every tensor a step mutates (used to make warm-up runs side-effect free)."""

    def __init__(self, tensors: List[torch.Tensor]):
        self.tensors = tensors
        self.saved = [t.detach().clone() for t in tensors]

    def restore(self):
        for t, s in zip(self.tensors, self.saved):
            t.copy_(s)


def capture_graph(fns, error_mode: str = "global"):
    """Capture ``fns`` (phase runs) into one HIP graph on the engine's capture stream.  Returns (graph,
    EventKeeper): the keeper holds the events the capture recorded and must live as long as the graph."""
    keeper = EventKeeper()
    g = torch.cuda.CUDAGraph()
    cap = EngineStreams.get(torch.cuda.current_stream().device).capture
    with keeper, torch.cuda.graph(g, stream=cap, capture_error_mode=error_mode):
        for f in fns:
            f()
    return g, keeper


@dataclasses.dataclass
class InferSource:
    """What a runner's inference graph (kind "infer" or "live") was built from.  Another tensor or another constant
    is another graph: the launches hold the device pointers and the constants."""
    tensors: Dict[str, torch.Tensor]  # by name; compared by identity
    consts: Dict[str, int]            # compared by value
    rollback: Tuple[str, ...]         # the tensors the step writes: a warm-up may not leave them changed
    phases: Callable                  # (program, source) -> (gather phase, store phase) around fwd_eval
    key: object = None                # what the source's owner knows it by (inference.resident_probs)

    def same(self, o: "InferSource") -> bool:
        return (self.tensors.keys() == o.tensors.keys() and all(t is o.tensors[k] for k, t in self.tensors.items())
                and self.consts == o.consts)


def _window_phases(p, s: InferSource):
    t = s.tensors
    by = {k: t[k] for k in ("sel", "count") if k in t}  # a gated source: rows numbered by the selection
    return (p.window_gather_phase(t["rec"], t["fs"], t["ts"], cursor=t["cursor"], **s.consts, **by),
            p.window_probs_phase(t["probs"], cursor=t["cursor"], **s.consts, **by))


def _live_phases(p, s: InferSource):
    t, c = s.tensors, s.consts
    by = {k: t[k] for k in ("sel", "count", "cursor") if k in t}  # a gated source: rows numbered by the selection
    return (p.live_gather_phase(t["ring"], t["fs"], t["state"], c["st"], **by),
            p.live_probs_phase(t["table"], t["state"], t["fs"].numel(), c["jcap"], **by))


class StepRunner:
    # Graphs are captured (and warmed up) on the engine's own capture stream (EngineStreams.capture), never on
    # torch's pool streams: the world > 1 data-parallel step ran 2.7x slower with pool capture streams (bench.py
    # --dp-shape 8 on Model A: 11.3 k -> 30.3 k samples/s, docs/PERF.md round 5).

    def __init__(self, program, X: torch.Tensor, labels: torch.Tensor, use_graph: bool = True,
                 allreduce: Optional[Callable[[torch.Tensor], None]] = None, X_eval: torch.Tensor = None,
                 labels_eval: torch.Tensor = None, resident: bool = True):
        self.p = program
        # False: the sources are a streaming ring whose rows change under the step (data/stream.py), not a
        # resident set -- the SNR noise, keyed by dataset row and scaled by a per-row power table, cannot serve it
        self.resident = resident
        self.use_graph = use_graph and program.device.type == "cuda"
        self.allreduce = allreduce
        B = program.B
        self.idx = torch.zeros(B, dtype=torch.int64, device=program.device)
        self.sources = {"train": (X, labels)}
        if X_eval is not None:
            self.sources["eval"] = (X_eval, labels_eval)
        self.graphs: Dict[str, torch.cuda.CUDAGraph] = {}
        self.keepers: Dict[str, EventKeeper] = {}  # events each graph was captured with (same lifetime)
        self._packed = False
        self._bwd_dp = None
        self._bwd_ext = None
        # the DP step as one graph with the bucket collectives captured in it (FlatGradAllReducer.capturable)
        self.capture_dp = self.use_graph and allreduce is not None and getattr(allreduce, "capturable", False)
        # otherwise forward + backward as one graph with an external event per gradient bucket, the bucket
        # all-reduces issued eagerly on the communication stream after those events (train_step)
        self.ext_dp = self.use_graph and allreduce is not None and not self.capture_dp
        self.ext_events = None
        reducing = allreduce is not None and getattr(getattr(allreduce, "ctx", None), "enabled", False)
        if reducing and any(l.is_early_adam for l in program.bwd.launches):
            # an update inside the backward would use local, un-reduced gradients
            raise ValueError("data-parallel step with weight updates inside the backward: call "
                             "set_optimizer(data_parallel=True) before autotune_program")
        if hasattr(program, "use_early_step_counter"):
            program.use_early_step_counter()  # the step counter off the step's tail (every step runs the forward)
        if hasattr(program, "check_sync_bn"):
            program.check_sync_bn()  # every SyncBN collective the program promised is in its launch lists
        self.buckets = list(program.buckets or [(0, program.flat.numel)])
        self.schedule = None  # [nrows][B] batch-index schedule (set_index_schedule)
        self.cursor = None
        # inference sources by graph kind: "infer" (set_window_source) and "live" (set_live_source)
        self.inference: Dict[str, InferSource] = {}
        self.window_cursor = None
        self.captures = 0  # graphs captured so far (a live source is captured once, whatever is pushed)
        # SNR noise in the gather (set_train_noise / set_eval_noise): per mode the launch constant (seed; None: off)
        # and the device scalars the captured graphs read -- fp32 (lo, hi) and the int64 draw number
        self.noise_seed = {"train": None, "eval": None}
        self.noise_snr = {k: torch.zeros(2, dtype=torch.float32, device=program.device) for k in ("train", "eval")}
        self.noise_draw = {k: torch.zeros(1, dtype=torch.int64, device=program.device) for k in ("train", "eval")}
        self._power = {}  # mode -> (X, its power table): cached by tensor identity

    def set_index_schedule(self, schedule: Optional[torch.Tensor]):
        """Train from a device-resident [nrows][B] batch-index schedule: ``train_step()`` without indices then
        gathers row (cursor mod nrows) and the step's optimizer kernel advances the cursor, so a replay is not
        preceded by a host-issued index copy (A: 6 us per step, tools/step_overhead.py).  The cursor restarts at
        row 0; None returns to per-call indices.  The training graphs are re-captured."""
        for kind in [k for k in self.graphs if k.startswith("train")]:
            self._drop_graph(kind)
        if schedule is None:
            self.schedule = self.cursor = None
            self.p.set_step_cursor(None)
            return
        if schedule.dim() != 2 or schedule.shape[1] != self.p.B or schedule.dtype != torch.int64:
            raise ValueError(f"index schedule must be int64 [nrows][{self.p.B}]")
        self.schedule = schedule.to(self.p.device).contiguous()
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.p.device)
        self.p.set_step_cursor(self.cursor)

    def restart_schedule(self, schedule: torch.Tensor):
        """Start the schedule over with new rows of the same shape (the next epoch): copied into the buffer the
        captured graphs read, cursor back to row 0, no re-capture."""
        if self.schedule is None or self.schedule.shape != schedule.shape:
            return self.set_index_schedule(schedule)
        self.schedule.copy_(schedule)
        self.cursor.zero_()

    # -------------------------------------------------------------------------------------------
    def _set_noise(self, mode: str, snr, seed: int, draw: Optional[int]):
        kinds = [k for k in self.graphs if k.startswith("train")] if mode == "train" else ["eval"]
        new_seed = None if snr is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        if snr is not None and not self.resident:
            raise ValueError("SNR noise needs a resident dataset: the streaming ring's rows (--dataset_ram False) "
                             "are not dataset rows")
        if new_seed != self.noise_seed[mode]:  # on, off or another seed (a launch constant): other launches
            for kind in kinds:
                self._drop_graph(kind)
            self.noise_seed[mode] = new_seed
        if snr is None:
            self._power.pop(mode, None)
            return
        lo, hi = parse_snr_range(snr)
        self.noise_snr[mode].copy_(torch.tensor([lo, hi], dtype=torch.float32))
        if draw is not None:
            self.noise_draw[mode].fill_(int(draw))
        self._noise_power(mode)

    def set_train_noise(self, snr, seed: int = 0, draw: Optional[int] = None):
        """Train on noisy inputs, fresh noise every step (csrc/augment.hip, data/noise.py): ``snr`` = (lo, hi) in dB
        -- every sample of every step draws its level uniformly from the range -- or None for the clean gather.
        The step's gather phase advances the draw number, so step k of a run sees draw d0 + k.  Turning the noise
        on or off (or another seed) drops the captured training graphs; another range only writes the device
        scalars they read.  ``draw``: restart the draw number (None keeps it)."""
        self._set_noise("train", snr, seed, draw)

    def set_eval_noise(self, snr_db: Optional[float], draw: int = 0, seed: int = EVAL_SEED):
        """Evaluate the (clean) eval source at a fixed SNR: the eval step's gather adds the evaluation noise of
        ``draw`` at ``snr_db`` dB, the same for every model and run; None returns to the clean gather.  Turning it
        on or off drops the captured eval graph; another level or draw only writes device scalars."""
        self._set_noise("eval", snr_db, seed, draw)

    def _noise_power(self, mode: str) -> torch.Tensor:
        """The power table of the mode's bound source, computed once per set (cached by tensor identity)."""
        from ..ops.functional import sample_power
        X = self.sources[mode if mode in self.sources else "train"][0]
        cur = next((c for c in self._power.values() if c[0] is X), None)  # (both modes may read one set)
        if cur is None:
            cur = (X, sample_power(X))
        self._power[mode] = cur
        return cur[1]

    def _noise_spec(self, mode: str) -> Optional[NoiseSpec]:
        if self.noise_seed[mode] is None:
            return None
        if not self.resident:
            raise ValueError("SNR noise needs a resident dataset")
        return NoiseSpec(self._noise_power(mode), self.noise_snr[mode], self.noise_draw[mode], self.noise_seed[mode],
                         train=mode == "train")

    def _mutable_state(self, kind: Optional[str] = None) -> List[torch.Tensor]:
        f = self.p.flat
        # an inference step advances its batch cursor (live: next) and fills rows of the probability table: a
        # warm-up that left either behind would skip the first batch
        src = self.inference.get(kind)
        infer = [src.tensors[k] for k in src.rollback] if src is not None else []
        return ([f.params, f.grads, f.exp_avg, f.exp_avg_sq, f.bn_mean, f.bn_var, f.bn_nbt, f.step, self.p.metrics,
                 self.p.confusion, self.p.logp] + list(self.p.extra_state)
                + ([self.cursor] if self.cursor is not None else []) + infer
                # the training gather phase advances the draw number: the first real step uses the draw that was set
                + ([self.noise_draw["train"]] if self.noise_seed["train"] is not None else []))

    def pack_weights(self):
        """(Re)build the bf16 MFMA weight images from the fp32 masters (after init / load_state_dict)."""
        self.p.opt["pack"].run()
        self._packed = True

    def _phases(self, kind: str) -> List[Callable[[], None]]:
        p = self.p
        if kind in self.inference:
            gather, store = self.inference[kind].phases(p, self.inference[kind])
            return [gather.run, p.fwd_eval.run, store.run]
        X, lab = self.sources["train" if kind.startswith("train") else "eval"]
        # a training step's gather also zeroes the arena's accumulators (one launch; arena.clear otherwise)
        sched = self.schedule is not None and kind.startswith("train")
        gather = p.gather_phase(X, lab, self.schedule if sched else self.idx, clear=kind.startswith("train"),
                                cursor=self.cursor if sched else None,
                                noise=self._noise_spec("train" if kind.startswith("train") else "eval"))
        if kind == "train_ext":
            if self._bwd_ext is None:
                self.ext_events = [ExtEvent() for _ in self.buckets]
                self._bwd_ext = p.backward_with_ext_events(self.ext_events)
            return [gather.run, p.fwd_train.run, self._bwd_ext.run]
        if kind == "train_compute":
            return [gather.run, p.fwd_train.run, p.bwd.run]
        if kind == "train_opt":
            return [p.opt["adam"].run]
        if kind == "train_full":
            return [gather.run, p.fwd_train.run, p.bwd.run, p.opt["adam"].run]
        if kind == "train_full_dp":
            if self._bwd_dp is None:
                self._bwd_dp = p.backward_with_allreduce(self.allreduce.ordered)
            return [gather.run, p.fwd_train.run, self._bwd_dp.run, p.opt["adam"].run]
        if kind == "eval":
            return [gather.run, p.fwd_eval.run]
        raise ValueError(kind)

    def _run(self, kind: str):
        if not self.use_graph:
            for f in self._phases(kind):
                f()
            return
        self._ensure_graph(kind)
        self.graphs[kind].replay()

    def _drop_graph(self, kind: str):
        """Release one captured graph and the events it was captured with, after the device has finished
        every replay of it (destroying an executable that may still run is undefined)."""
        g = self.graphs.pop(kind, None)
        if g is None:
            return
        torch.cuda.synchronize()
        g.reset()
        self.keepers.pop(kind, None)

    def _ensure_graph(self, kind: str):
        """Warm up (side effects rolled back) and capture the graph of ``kind`` once."""
        g = self.graphs.get(kind)
        if g is None:
            fns = self._phases(kind)
            snap = StateSnapshot(self._mutable_state(kind))
            s = EngineStreams.get(torch.cuda.current_stream().device).capture
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):  # warm-up (loads code objects); side effects are rolled back
                for f in fns:
                    f()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            snap.restore()
            self.p.opt["pack"].run()  # the bf16 weight images are derived state: rebuild from restored masters
            # Collectives captured here run on the capture-only RCCL communicator (DistContext.capture_group),
            # which never has eager work for the process-group watchdog to poll; the capture is thread-local
            # so that the watchdog's polls of the default communicator's eager work stay legal meanwhile.
            g, keeper = capture_graph(fns, "thread_local")
            torch.cuda.synchronize()
            self.graphs[kind] = g
            self.keepers[kind] = keeper
            self.captures += 1

    # -------------------------------------------------------------------------------------------
    def set_lr(self, lr: float):
        self.p.flat.lr.fill_(float(lr))

    def train_step(self, idx: Optional[torch.Tensor] = None):
        """One training step on the batch ``idx`` -- or, with an index schedule set (set_index_schedule) and
        no ``idx``, on the schedule's next row."""
        if not self._packed:
            self.pack_weights()
        if idx is not None:
            if self.schedule is not None:
                raise ValueError("an index schedule is set: call train_step() without indices")
            self.idx.copy_(idx, non_blocking=True)
        elif self.schedule is None:
            raise ValueError("train_step() without indices needs set_index_schedule")
        if self.allreduce is None:
            self._run("train_full")
        elif self.capture_dp:
            self._run("train_full_dp")
        elif self.ext_dp:
            # one graph for forward + backward; bucket k's all-reduce is issued on the communication stream
            # behind the graph's external event k, so it overlaps the rest of the backward
            if not self.graphs.get("train_ext") or not self.graphs.get("train_opt"):
                self._ensure_graph("train_ext")  # both captured before any collective is in flight (the
                self._ensure_graph("train_opt")  # capture's state snapshot/restore must not race an all-reduce)
            self._run("train_ext")
            g = self.p.flat.grads
            if hasattr(self.allreduce, "start"):
                comm = EngineStreams.get(self.p.device).comm
                for ev, (lo, hi) in zip(self.ext_events, self.buckets):
                    ev.wait(comm)
                    with torch.cuda.stream(comm):
                        self.allreduce.start(g[lo:hi])
                self.allreduce.finish()
            else:  # a plain callable: the whole gradient, in stream order after the graph
                self.allreduce(g)
            self._run("train_opt")
        else:  # eager launches (no graphs): the whole gradient after the backward
            self._run("train_compute")
            self.allreduce(self.p.flat.grads)
            self._run("train_opt")

    def set_eval_source(self, X: torch.Tensor, labels: torch.Tensor):
        """Point the eval step at another resident set (the captured eval graph is rebuilt when the
        tensors differ: its gather launch holds their device pointers)."""
        cur = self.sources.get("eval")
        if cur is not None and cur[0] is X and cur[1] is labels:
            return
        self.sources["eval"] = (X, labels)
        self._drop_graph("eval")
        if self.noise_seed["eval"] is not None:
            self._noise_power("eval")

    def eval_step(self, idx: torch.Tensor):
        if not self._packed:
            self.pack_weights()
        self.idx.copy_(idx, non_blocking=True)
        self._run("eval")

    def set_window_source(self, rec: torch.Tensor, fs: torch.Tensor, ts: torch.Tensor, probs: torch.Tensor,
                          lo: int = 0, hi: Optional[int] = None, key=None, sel: Optional[torch.Tensor] = None,
                          count: Optional[torch.Tensor] = None):
        """Resident-recording inference: ``infer_step()`` then evaluates the next ``B`` windows of ``[lo, hi)`` --
        cut on the device from ``rec`` [C, F, T] at the starts ``fs`` x ``ts`` (int32 device tables, window
        ``n = a * len(ts) + b``) -- and writes their probabilities into rows of ``probs`` [N, K]; the step's last
        kernel advances the batch cursor, so ceil((hi - lo) / B) calls cover the range with no host copy between
        them.  The cursor restarts at ``lo``.  Other tensors or another range rebuild the captured graph (its
        launches hold the device pointers and the range).  ``key``: kept as the source's ``key`` until it is
        replaced or cleared -- how a caller that uploaded the tensors recognises them again.

        ``sel`` / ``count`` (together): an on-device selection (ops.functional.select_windows) -- ``infer_step()``
        then evaluates the next ``B`` entries of ``sel`` (int64 window numbers of ``[lo, hi)``) below ``count``, a
        device int64 scalar that every replay reads: ceil(count / B) calls cover the selection, whatever it is, with
        one captured graph.  The two tensors are part of the source like the others."""
        hi = fs.numel() * ts.numel() if hi is None else hi
        if probs.shape[0] != fs.numel() * ts.numel():
            raise ValueError("the probability table needs one row per window")
        if not 0 <= lo <= hi <= probs.shape[0]:
            raise ValueError(f"window range [{lo}, {hi}) outside the {probs.shape[0]} windows")
        if (sel is None) != (count is None):
            raise ValueError("a selection is sel and count together")
        if self.window_cursor is None:
            self.window_cursor = torch.zeros(1, dtype=torch.int64, device=self.p.device)
        tensors = {"rec": rec, "fs": fs, "ts": ts, "probs": probs, "cursor": self.window_cursor}
        if sel is not None:
            tensors.update(sel=sel, count=count)
        self._set_source("infer", InferSource(tensors, {"lo": int(lo), "hi": int(hi)}, ("cursor", "probs"),
                                              _window_phases)).key = key
        self.window_cursor.zero_()

    def clear_window_source(self):
        """Release the window source (the recording and its table can be freed before the next one is uploaded)."""
        self._clear_source("infer")

    def infer_step(self):
        """One batch of the window source: [window gather, eval forward, probabilities + cursor], one graph."""
        self._source_ready("infer", "infer_step() needs set_window_source")
        self._run("infer")

    def set_live_source(self, ring: torch.Tensor, fs: torch.Tensor, state: torch.Tensor, table: torch.Tensor,
                        st: int, jcap: int, sel: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                        cursor: Optional[torch.Tensor] = None):
        """Live inference on a growing recording: ``live_step()`` then evaluates windows ``next .. next + B - 1`` of
        the time ring ``ring`` [C, F, R] -- window ``n = j * nf + a`` at ``(fs[a], j * st)``, those from ``avail`` on
        as padding -- and writes their probabilities to rows ``(j mod jcap) * nf + a`` of ``table``; the step's last
        kernel advances ``next`` by the valid rows.  ``state``: the device scalars (ops.functional.live_state) that
        ring_append advances as data arrives.  The graph is captured once per source: pushes, the wrap of the ring
        and the end of the stream only change device state.

        ``sel`` / ``count`` / ``cursor`` (together): a gated live source (ops.functional.live_select) --
        ``live_step()`` then evaluates the next ``B`` entries of ``sel`` below ``count``, both read on the device by
        every replay, into the gated table [>= jcap * nf, K + 1], and advances ``cursor``: ceil(count / B) calls
        cover the selection of a piece with the one captured graph.  The three tensors are part of the source."""
        tensors = {"ring": ring, "fs": fs, "state": state, "table": table}
        rollback = ("state", "table")
        if not (sel is None and count is None and cursor is None):
            if sel is None or count is None or cursor is None:
                raise ValueError("a live selection is sel, count and cursor together")
            tensors.update(sel=sel, count=count, cursor=cursor)
            rollback += ("cursor",)
        self._set_source("live", InferSource(tensors, {"st": int(st), "jcap": int(jcap)}, rollback, _live_phases))

    def clear_live_source(self):
        """Release the live source (its graph, and the runner's hold on the ring and the table)."""
        self._clear_source("live")

    def prepare_live(self):
        """Capture the live graph now (side effects rolled back), so that no push pays for it."""
        self._source_ready("live", "prepare_live() needs set_live_source")
        if self.use_graph:
            self._ensure_graph("live")

    def live_step(self):
        """One batch of the live source: [ring gather, eval forward, probabilities + next], one graph."""
        self._source_ready("live", "live_step() needs set_live_source")
        self._run("live")

    def _set_source(self, kind: str, new: InferSource) -> InferSource:
        """Bind an inference source; the kind's graph survives only if it was built from the same one."""
        cur = self.inference.get(kind)
        if cur is None or not cur.same(new):
            self._drop_graph(kind)
            self.inference[kind] = cur = new
        return cur

    def _clear_source(self, kind: str):
        self._drop_graph(kind)
        self.inference.pop(kind, None)

    def _source_ready(self, kind: str, unbound: str):
        if kind not in self.inference:
            raise ValueError(unbound)
        if not self._packed:
            self.pack_weights()

    def reset_metrics(self):
        self.p.metrics.zero_()
        self.p.confusion.zero_()

    def close(self):
        """Release every HIP object the runner and its program's phases hold -- graph executables with the
        events they were captured with, the phases' last eager events, the replay stream -- while the HIP runtime is certainly alive (at interpreter exit the
        order in which module globals, the runtime and these objects are finalised is not defined).  The
        runner can be used again afterwards (graphs are re-captured on demand)."""
        torch.cuda.synchronize()
        for k in list(self.graphs):
            self._drop_graph(k)
        p = self.p
        phases = [p.fwd_train, p.fwd_eval, p.bwd] + list(p.opt.values())
        phases += [ph for ph in (self._bwd_dp, self._bwd_ext) if ph is not None]
        for ph in phases:
            ph.release()
        self._bwd_dp = self._bwd_ext = None
        for ev in self.ext_events or []:
            ev.destroy()
        self.ext_events = None
        torch.cuda.synchronize()

"""Per-layer kernel autotuning on the device.

Every conv forward / data-gradient launch of a lowered program has 14 tile configurations
(csrc/conv.hip ``launch_conv_cfg``: wave layout channels x pixels x K-split).  The best one depends on
the layer's M (B*H*W), N (channels) and K (taps*Cin) and on MI355X's CU count, so it is *measured*:
each candidate is timed from a HIP graph of back-to-back launches (no host overhead), the fastest is
written into the launch, and the result is cached by shape signature in ``tuned_cfgs.json`` (shipped in
the package, so normal runs do not pay the tuning time).
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, Optional

import torch

from ..ops.functional import (CONV_DEEP_CFG0, CONV_DEEP_NCFG, CONV_GLDS_CFG0, CONV_GLDS_NCFG, CONV_LDS_CFG0,
                              CONV_LDS_NCFG, CONV_PATCH_CFG0, CONV_PATCH_NCFG, CONV_PATCHP_CFG0, CONV_PATCHP_NCFG,
                              CONV_XCD, GDEEP_TILES, WGRAD_PATCH, WGRAD_TILES, conv_workspace, glds_cfg, wgrad_big_cfg,
                              wgrad_family, wgrad_lean_twin)
from ..ops.hip import lib
from .program import EventKeeper

# conv.hip register-pipelined tiles 0-13 (pipeline depth 2, and 4 at CONV_DEEP_CFG0 + tile), then
# conv_lds.hip LDS-staged tiles x K chunk x K split, its LDS-DMA tiles x K split, the 3x3 / stride-1
# patch tiles x channel slice (one strip per block, and persistent), the deep-ring LDS-DMA tiles x K split
CONV_CFGS = (list(range(14)) + list(range(CONV_LDS_CFG0, CONV_LDS_CFG0 + CONV_LDS_NCFG))
             + list(range(CONV_DEEP_CFG0, CONV_DEEP_CFG0 + CONV_DEEP_NCFG))
             + list(range(CONV_GLDS_CFG0, CONV_GLDS_CFG0 + CONV_GLDS_NCFG))
             + list(range(CONV_PATCH_CFG0, CONV_PATCH_CFG0 + CONV_PATCH_NCFG))
             + [glds_cfg(t, s, deep=True) for t in GDEEP_TILES for s in (1, 2, 4, 8)]
             + list(range(CONV_PATCHP_CFG0, CONV_PATCHP_CFG0 + CONV_PATCHP_NCFG)))


def fused_max_m(kind: int) -> int:
    """csrc/bn.hip tail_bwd_fused_kernel: 1024 threads x <= 4 register-cached pixels (2 for ADD_RELU)."""
    return 1024 * (2 if kind == 4 else 4)
WGRAD_CFGS = sorted(WGRAD_TILES) + sorted(WGRAD_PATCH)
_CACHE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_cfgs.json")


def conv_signature(mode: int, G: int, d: dict) -> str:
    keys = ("B", "Hs", "Ws", "Ho", "Wo", "N", "Cs", "KH", "KW", "sh", "sw", "ph", "pw")
    src = d["src"]
    sig = f"conv{mode}|G{G}|" + ",".join(str(d[k]) for k in keys) + f"|seg{int(src.get('C1', 0) > 0)}" + \
          f"|st{int(bool(d.get('stats')))}"
    return sig


def wgrad_signature(G: int, d: dict) -> str:
    return "wgrad|" + conv_signature(0, G, dict(d, N=d["Co"], Hs=d["Hi"], Ws=d["Wi"], stats=0))


def load_cache(path: Optional[str] = None) -> Dict[str, int]:
    """The shipped table, or the one named by MDA_TUNED_CFGS (A/B runs of two tables on one box)."""
    named = path or os.environ.get("MDA_TUNED_CFGS")
    path = named or _CACHE_PATH
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError):
        if named:  # an explicitly named table that cannot be read must not silently become an empty one
            raise
        return {}


def save_cache(cache: Dict[str, int], path: str):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(sorted(cache.items())), f, indent=0)


def _time(fn, inner: int = 10, reps: int = 5) -> float:
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with EventKeeper() as keep, torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    g.reset()
    del g, keep
    return s.elapsed_time(e) / (inner * reps)


# isolated timings of every valid config of each measured conv signature (filled by autotune_phases,
# consumed by tune_in_context): sig -> [(ms, cfg)] ascending
ISOLATED: Dict[str, list] = {}


def _isolated(mode: int, G: int, d: dict, sig: str) -> list:
    """Isolated graph-replay time of every valid config of one conv launch (cached in ISOLATED)."""
    if sig in ISOLATED:
        return ISOLATED[sig]
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = []
    for c in CONV_CFGS:
        dc = dict(d)
        ws = conv_workspace(mode, c, G, dc, dev)
        if ws is None:
            continue
        res.append((_time(lambda: L.conv(mode, c, G, torch.cuda.current_stream().cuda_stream, dc)), c))
        del ws
    res.sort()
    ISOLATED[sig] = res
    return res


def autotune_phases(phases: Iterable, cache: Optional[Dict[str, int]] = None, verbose: bool = False,
                    measure: bool = True) -> Dict[str, int]:
    """Choose the conv tile config of every conv launch in ``phases`` (mutates the launches).  With
    ``measure=False`` only cached choices are applied (layers missing from the cache keep the heuristic)."""
    cache = load_cache() if cache is None else cache
    L = lib()
    for ph in phases:
        for launch in ph.launches:
            if not launch.is_conv:
                continue
            mode, cfg, G, d = launch.args
            sig = conv_signature(mode, G, d)
            if sig not in cache and not measure:
                continue
            if sig not in cache:
                best_t, best = _isolated(mode, G, d, sig)[0]
                cache[sig] = best
                if verbose:
                    print(f"tuned {sig}: cfg {best} ({best_t * 1e3:.1f} us)", flush=True)
            cfg = cache[sig]
            ws = conv_workspace(mode, cfg, G, d, torch.device("cuda", torch.cuda.current_device()))
            if ws is None:
                raise RuntimeError(f"cached conv config {cfg} is invalid for {sig}")
            ph.ws_keep[id(launch)] = ws  # split-K workspace of the chosen LDS config
            launch.set_cfg(cfg)
    for ph in phases:
        for launch in ph.launches:
            if not launch.is_wgrad or launch.owner is None:
                continue
            cfg, G, d = launch.args
            sig = wgrad_signature(G, d)
            if sig not in cache and not measure:
                continue
            if sig not in cache:
                best, best_t = cfg, float("inf")
                for c in WGRAD_CFGS:
                    if not launch.owner.wgrad_valid(c):
                        continue
                    launch.set_cfg(c)
                    t = _time(lambda: L.wgrad(c, G, torch.cuda.current_stream().cuda_stream, d))
                    if t < best_t:
                        best, best_t = c, t
                cache[sig] = best
                if verbose:
                    print(f"tuned {sig}: cfg {best} ({best_t * 1e3:.1f} us)", flush=True)
            launch.set_cfg(cache[sig])
    # BN backward: reduce + apply (grid over pixels, replica atomics) vs the single-launch variant
    # (one block per 8 channels over all pixels) -- the crossover depends on M, C and the sources
    for ph in phases:
        for launch in ph.launches:
            if not launch.is_tail_bwd:
                continue
            kind, G, blocks, d = launch.args
            if d.get("fused") in (2, 3):  # statistics from the producers (apply only) / a partial reduce
                continue
            sig = tail_bwd_signature(kind, G, d)
            if sig not in cache and not measure:
                continue
            if sig not in cache:
                fusable = d["B"] * d["H"] * d["W"] <= fused_max_m(kind)
                ts = [_time(lambda: L.tail_bwd(kind, G, blocks, torch.cuda.current_stream().cuda_stream,
                                                dict(d, fused=f))) if (f == 0 or fusable) else float("inf")
                      for f in (0, 1)]
                cache[sig] = int(ts[1] < ts[0])
                if verbose:
                    print(f"tuned {sig}: fused={cache[sig]} ({ts[0] * 1e3:.1f} / {ts[1] * 1e3:.1f} us)", flush=True)
            d["fused"] = cache[sig]
    return cache


def tail_bwd_signature(kind: int, G: int, d: dict) -> str:
    return (f"tailbwd|k{kind}|G{G}|{d['B']},{d['H']},{d['W']},{d['C']}|src{len(d['g'])}"
            f"|bn2{int('bn2' in d)}|side{int(bool(d.get('side')))}")


def spill_signature(prog) -> str:
    return f"wgspill|{type(prog).__name__}|B{prog.B}|convs{len(prog.convs)}"


def wgrad_spill_frac(prog, cache: Dict[str, int]) -> float:
    """Share of stream 0's weight-gradient work moved to the spill stream (LoweredProgram.spill_wgrads), in
    percent in the table (chosen in the captured step by tune_in_context); MDA_WGSPILL overrides."""
    env = os.environ.get("MDA_WGSPILL")
    if env is not None:
        return float(env)
    return cache.get(spill_signature(prog), 0) / 100.0


def autotune_program(prog, out_path: Optional[str] = None, verbose: bool = False, measure: bool = True,
                     batch_wgrads: bool = True, cache: Optional[Dict[str, int]] = None) -> Dict[str, int]:
    """Tune every conv launch of a lowered program (train forward, eval forward, backward), then batch the
    weight-gradient launches per tile config (``batch_wgrads``).  ``cache``: the table to use (default: the
    shipped one; empty with MDA_RETUNE=1)."""
    if prog.device.type != "cuda":
        return {}
    if cache is None:
        cache = {} if os.environ.get("MDA_RETUNE") == "1" else load_cache()
    n0 = len(cache)
    autotune_phases([prog.fwd_train, prog.fwd_eval, prog.bwd], cache, verbose, measure)
    if batch_wgrads:
        prog.batch_tails()
        prog.spill_wgrads(wgrad_spill_frac(prog, cache))
        prog.merge_wgrad_cfgs()
    prog.refresh_wgrad_finalize()
    if batch_wgrads:
        prog.batch_wgrads()
    if out_path and len(cache) != n0:
        save_cache(cache, out_path)
    return cache


def _wgrad_groups(prog) -> tuple:
    """(per-conv weight-gradient launches, the same grouped by signature, signature -> work of its group)."""
    wg = [l for l in prog.bwd.launches if l.is_wgrad and l.owner is not None]
    groups: Dict[str, list] = {}
    for l in wg:
        groups.setdefault(wgrad_signature(l.G, l.d), []).append(l)

    def weight(sig):
        d = groups[sig][0].d
        return len(groups[sig]) * d["B"] * d["Ho"] * d["Wo"] * d["Npad"] * d["Kpad"]
    return wg, groups, weight


def tune_wgrad_batches(prog, cache: Dict[str, int], verbose: bool = False, passes: int = 1,
                       init_big: bool = False, init_lean=False) -> Dict[str, int]:
    """Choose the weight-gradient configs by the time of the BATCHED launches they end up in.

    A conv's weight gradient never runs alone: it is a job of one batched launch per (stream, config)
    (engine/lowering.py batch_wgrads) beside dozens of others, so what counts is the aggregate -- bytes
    staged through LDS, blocks in flight, the finalize's split-slab reads -- not one job's latency, which
    is what the isolated timing of autotune_phases ranks (it favours small tiles with many blocks; in the
    batch the large 32x32x16 tiles, 2-4x fewer staged bytes per output, win on the big layers).  Greedy
    coordinate descent over the wgrad signatures (costliest first): each valid config is applied, the
    per-stream config cap (merge_wgrad_cfgs) and the finalize refresh run as the bench runs them, and the
    sum of the batched launches' and the finalize's isolated graph-replay times decides.  ``init_big``:
    start from every im2col conv on the large tile its shape suits (patch configs kept) -- one batch per
    stream -- instead of the table's choices.  Must run before batch_wgrads (on the per-conv launches).
    Updates and returns ``cache``."""
    L = lib()
    wg, groups, weight = _wgrad_groups(prog)
    if not wg:
        return cache
    assign = {sig: ls[0].cfg for sig, ls in groups.items()}
    fin = [l for l in prog.bwd.launches if l.is_finalize]

    def cost() -> float:
        for sig, ls in groups.items():
            for l in ls:
                l.set_cfg(assign[sig])
        prog.merge_wgrad_cfgs()
        prog.refresh_wgrad_finalize()
        total, n_kept = 0.0, len(prog.keep_alive)
        for bk, st in sorted({(l.bucket, l.stream) for l in wg}):
            mine = [l for l in wg if (l.bucket, l.stream) == (bk, st)]
            for b in prog._batch_stream_wgrads(mine, st, [], "", bk)[1]:
                cfg, t, n, nb, _ = b.args  # timed on an uncapped grid (one block per virtual block)
                total += _time(lambda: L.wgrad_batched(cfg, t.data_ptr(), n, nb,
                                                       torch.cuda.current_stream().cuda_stream, 0))
        del prog.keep_alive[n_kept:]  # the timed job tables; the launches keep their per-conv form
        for f in fin:
            total += _time(lambda f=f: f.fn(*f.args, torch.cuda.current_stream().cuda_stream))
        return total

    t0 = cost()
    if init_lean:  # signatures on their fastest lean-staging config, timed alone (csrc/wgrad_lean.hip); a set of
        # streams restricts it to the weight gradients batched on those streams
        for sig, ls in groups.items():
            l0 = ls[0]
            if init_lean is not True and l0.stream not in init_lean:
                continue
            cand = []
            for c in [c for c in WGRAD_CFGS if wgrad_family(c) == "lean"]:
                if not all(l.owner.wgrad_valid(c) for l in ls):
                    continue
                l0.set_cfg(c)
                cand.append((_time(lambda c=c: L.wgrad(c, l0.G, torch.cuda.current_stream().cuda_stream, l0.d)), c))
            l0.set_cfg(assign[sig])
            if cand:
                assign[sig] = min(cand)[1]
    if init_big:
        for sig, ls in groups.items():
            c = wgrad_big_cfg(ls[0].owner.Npad, ls[0].owner.Kpad_w)
            if wgrad_family(assign[sig]) != "patch" and all(l.owner.wgrad_valid(c) for l in ls):
                assign[sig] = c
    best = cost()
    for _ in range(passes):
        changed = False
        for sig in sorted(groups, key=weight, reverse=True):
            cur = assign[sig]
            for c in WGRAD_CFGS:
                if c == assign[sig] or not all(l.owner.wgrad_valid(c) for l in groups[sig]):
                    continue
                prev = assign[sig]
                assign[sig] = c
                t = cost()
                if t < best * 0.995:
                    best = t
                    changed = True
                else:
                    assign[sig] = prev
            if assign[sig] != cur and verbose:
                print(f"  {sig}: wgrad cfg {cur} -> {assign[sig]} (batches + finalize {best * 1e3:.1f} us)",
                      flush=True)
        if not changed:
            break
    cost()  # leave the launches on the chosen assignment
    cache.update(assign)
    if verbose:
        print(f"wgrad batches + finalize: {t0 * 1e3:.1f} -> {best * 1e3:.1f} us", flush=True)
    return cache


def tune_wgrad_in_step(make_prog, X: torch.Tensor, labels: torch.Tensor, cache: Dict[str, int], top: int = 10,
                       topk: int = 3, margin: float = 0.003, verbose: bool = True) -> Dict[str, int]:
    """Choose the weight-gradient configs of the ``top`` heaviest weight-gradient signatures by the time of
    the WHOLE captured training step (the isolated ranking favours the tile with the most
    blocks, and the batch-level ranking of tune_wgrad_batches times the batches alone -- on Model A neither
    reproduces the step-level choice).  The batched launches are built from the per-conv choices, so every
    candidate gets its own lowering: ``make_prog()`` builds a fresh, un-tuned program.  Candidates per
    signature: the ``topk`` configs of the isolated ranking and the signature's large-tile config; one is
    kept when two re-timings both beat the incumbent (re-timed right before) by ``margin``.  Updates and
    returns ``cache``."""
    L = lib()
    base = make_prog()
    wg, groups, weight = _wgrad_groups(base)
    order = sorted(groups, key=weight, reverse=True)[:top]
    ranked = {}
    for sig in order:  # isolated ranking of the signature's valid configs (first launch of the group)
        l = groups[sig][0]
        cfg0, G, d = l.args
        conv, res = l.owner, []
        for c in WGRAD_CFGS:
            if all(k.owner.wgrad_valid(c) for k in groups[sig]):
                l.set_cfg(c)
                res.append((_time(lambda c=c: L.wgrad(c, G, torch.cuda.current_stream().cuda_stream, d)), c))
        l.set_cfg(cfg0)
        res.sort()
        big = wgrad_big_cfg(conv.Npad, conv.Kpad_w)
        cands = [c for _, c in res[:topk]]
        for c in (big, wgrad_lean_twin(big)):  # the large tile and its lean-staging form
            if c in {c2 for _, c2 in res} and c not in cands:
                cands.append(c)
        ranked[sig] = cands
    del base
    torch.cuda.empty_cache()

    def step_with(over: Dict[str, int]) -> float:
        prog = make_prog()
        cc = dict(cache)
        cc.update(over)
        autotune_program(prog, cache=cc, measure=False)
        t = step_time_us(prog, X, labels, reps=40, rounds=3)
        del prog
        torch.cuda.empty_cache()
        return t

    start = {sig: cache.get(sig) for sig in order}
    t0 = step_with({})
    for sig in order:
        cur = cache.get(sig)
        for c in ranked[sig]:
            if c == cache.get(sig):
                continue
            t_inc = step_with({})
            t = step_with({sig: c})
            if t < t_inc * (1.0 - margin) and step_with({sig: c}) < step_with({}) * (1.0 - margin):
                cache[sig] = c
                if verbose:
                    print(f"  {sig}: wgrad cfg {cur} -> {c}, step {t:.1f} us (incumbent {t_inc:.1f})", flush=True)
    changed = {sig: cache[sig] for sig in order if cache.get(sig) != start[sig]}
    if changed:
        # closing confirmation, as in tune_in_context: the accepted set against the starting one, interleaved;
        # a set that does not win 2 of 3 rounds is drift of the per-candidate re-timings -- revert it
        back = {sig: start[sig] for sig in changed if start[sig] is not None}
        wins = 0
        for _ in range(3):
            ts, tt = step_with(back), step_with({})
            wins += tt < ts
            if verbose:
                print(f"  confirmation: start configs {ts:.1f} us, tuned {tt:.1f} us", flush=True)
        if wins < 2:
            for sig in changed:
                if start[sig] is None:
                    cache.pop(sig, None)
                else:
                    cache[sig] = start[sig]
            if verbose:
                print(f"weight gradients in the step: {len(changed)} changes not confirmed -- reverted", flush=True)
    if verbose:
        print(f"weight gradients in the step: {t0:.1f} -> {step_with({}):.1f} us", flush=True)
    return cache


def _snapshot(prog):
    """The program's mutable state (restored after a timing run that trains at learning rate 0)."""
    from .step import StateSnapshot
    f = prog.flat
    return StateSnapshot([f.params, f.grads, f.exp_avg, f.exp_avg_sq, f.bn_mean, f.bn_var, f.bn_nbt, f.step,
                          f.lr, prog.metrics, prog.confusion, prog.logp] + list(prog.extra_state))


def _graph_ms(fns, reps: int, rounds: int, warm: int = 1) -> float:
    """Best-of-``rounds`` mean replay time (ms) of ``fns`` captured as one HIP graph, after one eager pass (the
    code objects of a new config are loaded before the capture) and ``warm`` replays."""
    from .step import capture_graph
    for fn_ in fns:
        fn_()
    torch.cuda.synchronize()
    g, events = capture_graph(fns)
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / reps)
    g.reset()  # release the graph and its executable now (hundreds of captures per tuning run)
    del g, events
    return best


def step_time_us(prog, X: torch.Tensor, labels: torch.Tensor, reps: int = 100, rounds: int = 3) -> float:
    """Best-of-``rounds`` mean time of the training step (gather, forward, backward, Adam + re-pack at
    learning rate 0) captured as one HIP graph; the program's mutable state is restored afterwards."""
    snap = _snapshot(prog)
    prog.flat.lr.zero_()
    prog.opt["pack"].run()
    idx = torch.arange(prog.B, device=prog.device) % X.shape[0]
    gather = prog.gather_phase(X, labels, idx, clear=True)
    best = 1e3 * _graph_ms([gather.run, prog.fwd_train.run, prog.bwd.run, prog.opt["adam"].run], reps, rounds, warm=10)
    snap.restore()
    prog.opt["pack"].run()
    torch.cuda.synchronize()
    return best


def tune_spill(make_prog, X: torch.Tensor, labels: torch.Tensor, cache: Dict[str, int],
               fracs=(0, 50, 70, 90), margin: float = 0.005, verbose: bool = True) -> Dict[str, int]:
    """Choose the weight-gradient spill fraction (LoweredProgram.spill_wgrads; table entry in percent) by
    the captured step's time.  ``make_prog()`` builds a fresh, un-tuned program of the model (the spill
    rewrites the per-conv launches, which batching removes, so every candidate needs its own lowering).
    Candidates are timed in two alternating rounds and a fraction must beat 0 (off) by ``margin`` in
    both."""
    times: Dict[int, list] = {fr: [] for fr in fracs}
    key = None
    for _ in range(2):
        for fr in fracs:
            prog = make_prog()
            key = spill_signature(prog)
            cache[key] = fr
            autotune_program(prog, cache=cache, measure=False)
            times[fr].append(step_time_us(prog, X, labels))
            del prog
            torch.cuda.empty_cache()
    best = 0
    for fr in fracs:
        if fr and all(t < b * (1.0 - margin) for t, b in zip(times[fr], times[0])):
            if best == 0 or sum(times[fr]) < sum(times[best]):
                best = fr
    cache[key] = best
    if verbose:
        print("spill fractions: " + ", ".join(f"{fr}%: {' / '.join(f'{t:.1f}' for t in times[fr])} us"
                                              for fr in fracs) + f" -> {best}%", flush=True)
    return cache


def _set_conv_cfg(launch, cfg: int, keep: dict) -> bool:
    """Point a conv launch at ``cfg`` (attaching its split-K workspace); False when cfg cannot run it."""
    mode, _, G, d = launch.args
    dc = dict(d)
    ws = conv_workspace(mode, cfg, G, dc, torch.device("cuda", torch.cuda.current_device()))
    if ws is None:
        return False
    keep[id(launch)] = ws
    launch.set_cfg(cfg, dc)
    return True


def tune_in_context(prog, X: torch.Tensor, labels: torch.Tensor, cache: Dict[str, int], topk: int = 3,
                    reps: int = 15, rounds: int = 3, margin: float = 0.002, verbose: bool = True,
                    on_change=None, cfg_pass: bool = True, xcd_pass: bool = True,
                    tail_pass: bool = True, confirm_rounds: int = 3) -> Dict[str, int]:
    """Refine the conv configs (and the BN-tail backward variants) of a lowered program by timing the WHOLE
    training step, not the isolated launch.

    The isolated timings of ``autotune_phases`` are taken with L2-hot operands and no neighbours; inside the
    multi-stream step graph the same kernels overlap other streams and read operands other kernels just
    wrote, and run up to 2x longer (docs/PERF.md).  Here the step (gather, forward, backward with the batched
    weight gradients, Adam + re-pack, learning rate 0) is captured as one HIP graph and replayed; for every
    conv signature (all launches sharing it change together, so the table stays one config per signature),
    largest isolated time first, each of its ``topk`` best isolated configs is tried and kept when the
    replayed step gets faster by more than ``margin``; finally the whole tuned set must beat the starting
    choices in ``confirm_rounds`` interleaved re-timings, or it is reverted.  The program's mutable state is
    restored afterwards.  Updates and returns ``cache``."""
    snap = _snapshot(prog)
    prog.flat.lr.zero_()
    idx = torch.arange(prog.B, device=prog.device) % X.shape[0]
    gather = prog.gather_phase(X, labels, idx, clear=True)
    fns = [gather.run, prog.fwd_train.run, prog.bwd.run, prog.opt["adam"].run]
    keep = {}

    def step_ms() -> float:
        return _graph_ms(fns, reps, rounds)

    groups: Dict[str, list] = {}
    for ph in (prog.fwd_train, prog.bwd):
        for l in ph.launches:
            if l.is_conv:
                mode, cfg, G, d = l.args
                groups.setdefault(conv_signature(mode, G, d), []).append(l)
    order = []
    for sig, ls in groups.items():
        mode, cfg, G, d = ls[0].args
        iso = _isolated(mode, G, d, sig)
        cur = next((t for t, c in iso if c == cfg & ~CONV_XCD), iso[0][0] if iso else 0.0)
        order.append((cur * len(ls), sig))
    order.sort(reverse=True)
    # the starting choices, for the closing confirmation (every accepted toggle beat the incumbent measured
    # right before it, but many toggles at a small margin can still add up to drift -- round 4 accepted 24
    # changes whose sum was 1.9 % SLOWER)
    start_cfg = {id(l): l.cfg for ls in groups.values() for l in ls}
    start_fused = {id(l): l.d.get("fused", 0) for l in prog.bwd.launches if l.is_tail_bwd}
    cache_before = dict(cache)
    base = step_ms()
    t0 = base
    if verbose:
        print(f"in-context tuning: {len(groups)} conv signatures, step {base * 1e3:.1f} us", flush=True)
    # every candidate is compared with the incumbent measured right before it: the step time drifts over
    # a minutes-long run (clocks, thermals), and a stale baseline credits that drift to whichever candidate
    # happens to be timed (a first version of this tuner "gained" 10 % that the benchmark did not show)
    for _, sig in (order if cfg_pass else []):
        ls = groups[sig]
        mode, cur, G, d = ls[0].args
        flag = cur & CONV_XCD  # the tile order is decided by its own pass below
        cands = [c | flag for _, c in _isolated(mode, G, d, sig)[:topk] if c | flag != cur]
        best_cfg = cur
        for c in cands:
            t_inc = step_ms()
            if not all(_set_conv_cfg(l, c, keep) for l in ls):
                for l in ls:
                    _set_conv_cfg(l, best_cfg, keep)
                continue
            t = step_ms()
            if t < t_inc * (1.0 - margin) and step_ms() < t_inc * (1.0 - margin):  # confirmed twice
                base, best_cfg = t, c
            else:
                for l in ls:
                    _set_conv_cfg(l, best_cfg, keep)
        if best_cfg != cur:
            cache[sig] = best_cfg
            if verbose:
                print(f"  {sig}: cfg {cur} -> {best_cfg}, step {base * 1e3:.1f} us", flush=True)
            if on_change is not None:
                on_change(cache)
    # tile order: every signature's config with the XCD-contiguous block order toggled (csrc/common.h
    # block_coords; it pays where neighbouring tiles share halo rows through one L2 -- only measurable in the
    # step, where the operands come from other kernels' writes, not from an L2-hot isolated replay)
    if xcd_pass:
        for _, sig in order:
            ls = groups[sig]
            cur = ls[0].cfg
            t_inc = step_ms()
            if not all(_set_conv_cfg(l, cur ^ CONV_XCD, keep) for l in ls):
                for l in ls:
                    _set_conv_cfg(l, cur, keep)
                continue
            t = step_ms()
            if t < t_inc * (1.0 - margin) and step_ms() < t_inc * (1.0 - margin):
                base = t
                cache[sig] = cur ^ CONV_XCD
                if verbose:
                    print(f"  {sig}: xcd order {int(bool(cur & CONV_XCD))} -> {int(not cur & CONV_XCD)}, "
                          f"step {base * 1e3:.1f} us", flush=True)
                if on_change is not None:
                    on_change(cache)
            else:
                for l in ls:
                    _set_conv_cfg(l, cur, keep)
    # BN-tail backward variants (reduce + apply vs the single-launch kernel), chosen in isolation by
    # autotune_phases, re-decided in the step the same way
    tails: Dict[str, list] = {}
    for l in prog.bwd.launches:
        if l.is_tail_bwd and l.d.get("fused", 0) in (0, 1):
            kind, G, blocks, d = l.args
            tails.setdefault(tail_bwd_signature(kind, G, d), []).append(l)
    for sig, ls in (tails.items() if tail_pass else []):
        kind, G, blocks, d = ls[0].args
        cur = d.get("fused", 0)
        alt = 1 - cur
        if alt == 1 and (d["B"] * d["H"] * d["W"] > fused_max_m(kind) or d.get("gscale", 1.0) != 1.0):
            continue
        t_inc = step_ms()
        for l in ls:
            l.d["fused"] = alt
        t = step_ms()
        if t < t_inc * (1.0 - margin) and step_ms() < t_inc * (1.0 - margin):
            base = t
            cache[sig] = alt
            if verbose:
                print(f"  {sig}: fused {cur} -> {alt}, step {base * 1e3:.1f} us", flush=True)
            if on_change is not None:
                on_change(cache)
        else:
            for l in ls:
                l.d["fused"] = cur
    # closing confirmation: the final choices against the starting ones, interleaved rounds; the tuned set is
    # kept only if it is faster in every round by ``margin`` (else the starting table is restored)
    changed = [l for ls in groups.values() for l in ls if l.cfg != start_cfg[id(l)]]
    ch_tails = [l for l in prog.bwd.launches if l.is_tail_bwd
                and l.d.get("fused", 0) != start_fused.get(id(l), l.d.get("fused", 0))]
    if changed or ch_tails:
        final_cfg = {id(l): l.cfg for l in changed}
        final_fused = {id(l): l.d.get("fused", 0) for l in ch_tails}

        def apply(start: bool):
            for l in changed:
                _set_conv_cfg(l, start_cfg[id(l)] if start else final_cfg[id(l)], keep)
            for l in ch_tails:
                l.d["fused"] = start_fused[id(l)] if start else final_fused[id(l)]
        wins = []
        for _ in range(confirm_rounds):
            apply(True)
            t_start = step_ms()
            apply(False)
            t_final = step_ms()
            wins.append(t_final < t_start * (1.0 - margin))
            if verbose:
                print(f"  confirmation: start table {t_start * 1e3:.1f} us, tuned {t_final * 1e3:.1f} us", flush=True)
        if not all(wins):
            apply(True)
            cache.clear()
            cache.update(cache_before)
            base = t0
            if verbose:
                print(f"in-context tuning: {len(changed)} conv / {len(ch_tails)} tail changes not confirmed "
                      f"against the starting table -- reverted", flush=True)
    for ph in (prog.fwd_train, prog.bwd, prog.fwd_eval):
        ph.ws_keep.update(keep)
    if verbose:
        print(f"in-context tuning: step {t0 * 1e3:.1f} -> {base * 1e3:.1f} us", flush=True)
    snap.restore()
    prog.opt["pack"].run()
    torch.cuda.synchronize()
    return cache

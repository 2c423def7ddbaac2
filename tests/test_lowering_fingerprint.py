"""Lowering is bookkeeping: the launch lists a program lowers to are compared, hash by hash, with the lists the
same cases lowered to when ``tests/golden/lowering/fingerprints.json`` was recorded.

Every launch of ``fwd_train``, ``fwd_eval``, ``bwd``, ``opt["adam"]`` and of a derived backward phase is dumped
as phase name, launch name, ``fn.__name__``, logical stream, waits, record, bucket, owner type and arguments.
Arguments are canonical: dict keys sorted, every integer >= 2**32 (a pointer) replaced by ``p<k>`` in order of
first appearance within the phase (aliasing between arguments is kept, addresses are not), tensors by shape and
dtype, other objects by type name.  Each phase's event alias map and kept-workspace count, and per case the
buckets, ``num_launches()``, the pass counters and ``opt_segs``, are dumped too.  One SHA-256 per (case, phase).

The goldens are recorded from the commit BEFORE a change to the lowering, never from the code under test:

    python tests/test_lowering_fingerprint.py --write             # CPU cases -> fingerprints.json
    python tests/test_lowering_fingerprint.py --write --gpu       # tuned case, on an MI355X -> fingerprints_gpu.json
    python tests/test_lowering_fingerprint.py --dump DIR [--gpu]  # the full canonical dumps, one file per phase

A refactor must leave every hash as it is.  After an INTENDED change of the lowering, check out the parent, run
``--dump before/``, check out the change, run ``--dump after/``, read ``diff -r before after`` -- it shows the
launches that moved, appeared or changed arguments -- and only then record the new hashes with ``--write``.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowering")
GOLDEN_CPU = os.path.join(GOLDEN_DIR, "fingerprints.json")
GOLDEN_GPU = os.path.join(GOLDEN_DIR, "fingerprints_gpu.json")

PROGRAMS = ("A", "event", "distance", "C")
VARIANTS = ("plain", "spill", "cut", "syncext")
CASES = [f"{p}/{v}" for p in PROGRAMS for v in VARIANTS] + ["C/reorder"]
GPU_CASE = "A/tuned"
# switches of the lowering read from the environment: a case lowers with none of them set
_ENV = ("MDA_NOL", "MDA_FOLD", "MDA_HFUSE", "MDA_TAIL_BATCH", "MDA_WGSPILL", "MDA_BUCKETS", "MDA_TUNED_CFGS",
        "MDA_RETUNE")


def _noop(t):
    pass


class _Event:
    """Placeholder for an external event: backward_with_ext_events only stores it."""


def _program(name, device, **kw):
    from mtl_das_pytorch_amd.engine.inception import InceptionProgram
    from mtl_das_pytorch_amd.engine.mtl import MTLProgram
    from mtl_das_pytorch_amd.models import MTL_Net, Multi_Classifier, Single_Task_Net
    torch.manual_seed(0)
    if name == "A":
        return MTLProgram(MTL_Net(), 32, device, **kw)
    if name == "C":
        return InceptionProgram(Multi_Classifier(), 4, device, **kw)
    return MTLProgram(Single_Task_Net(name), 8, device, **kw)


def _passes(p, spill=0.0):
    p.batch_tails()
    p.spill_wgrads(spill)
    p.merge_wgrad_cfgs()
    p.refresh_wgrad_finalize()
    p.batch_wgrads()


def build_case(case, device="cpu"):
    """(program, derived backward phases) of one case."""
    name, variant = case.split("/")
    derived = []
    if variant in ("plain", "spill"):
        p = _program(name, device)
        p.segment_backward(1)
        _passes(p, 0.7 if variant == "spill" else 0.0)
    elif variant == "cut":
        p = _program(name, device)
        p.set_optimizer(grad_scale=0.5, data_parallel=True)
        p.segment_backward(2)
        _passes(p)
        derived.append(p.backward_with_allreduce(_noop))
    elif variant == "syncext":
        p = _program(name, device, sync_world=2)
        p.enable_sync_bn(_noop)
        p.set_optimizer(grad_scale=0.5, data_parallel=True)
        p.segment_backward(1)
        _passes(p)
        buckets = p.stream_buckets(2)
        derived.append(p.backward_with_ext_events([_Event() for _ in buckets]))
        p.use_early_step_counter()
        if hasattr(p, "check_sync_bn"):
            p.check_sync_bn()
    elif variant == "reorder":  # as test_stream_param_order_gives_model_c_side_stream_buckets
        from mtl_das_pytorch_amd.engine.inception import InceptionProgram
        from mtl_das_pytorch_amd.models import build_model
        model = build_model("multi_classifier")

        def make(order):
            torch.manual_seed(0)
            q = InceptionProgram(model, 8, device, param_order=order)
            q.set_optimizer(weight_decay=1e-5, data_parallel=True)
            q.segment_backward(1)
            q.merge_wgrad_cfgs()
            q.refresh_wgrad_finalize()
            q.batch_wgrads()
            q.batch_tails()
            return q

        torch.manual_seed(0)
        p = make(make(None).stream_param_order())
        p.stream_buckets(4)
    elif variant == "tuned":
        from mtl_das_pytorch_amd.engine.tune import autotune_program
        p = _program(name, device)
        p.segment_backward(1)
        autotune_program(p, measure=False)
    else:
        raise ValueError(case)
    return p, derived


class _Canon:
    """Canonical form of launch arguments; one instance per phase (the pointer numbering is the phase's)."""

    def __init__(self):
        self.ptrs = {}

    def __call__(self, o):
        if isinstance(o, bool) or o is None or isinstance(o, str):
            return o
        if isinstance(o, int):
            if o >= 1 << 32:
                return self.ptrs.setdefault(o, f"p{len(self.ptrs)}")
            return o
        if isinstance(o, float):
            return repr(o)
        if isinstance(o, dict):
            return {str(k): self(o[k]) for k in sorted(o, key=str)}
        if isinstance(o, (list, tuple)):
            return [self(v) for v in o]
        if isinstance(o, torch.Tensor):
            return f"tensor{list(o.shape)}:{o.dtype}"
        return type(o).__name__


def dump_phase(ph) -> str:
    canon = _Canon()
    lines = []
    for l in ph.launches:
        owner = type(l.owner).__name__
        if isinstance(l.owner, (list, tuple)):
            owner += f"[{len(l.owner)}]"
        lines.append(json.dumps([ph.name, l.name, getattr(l.fn, "__name__", None), l.stream, list(l.waits), l.record,
                                 l.bucket, owner, canon(l.args)], sort_keys=True))
    lines.append(json.dumps({"alias": dict(sorted(ph.alias.items())),
                             "ws_keep": len(getattr(ph, "ws_keep", None) or {})}, sort_keys=True))
    return "\n".join(lines) + "\n"


def dump_case(case, device="cpu") -> dict:
    """phase name (or "meta") -> canonical text."""
    saved = {k: os.environ.pop(k) for k in _ENV if k in os.environ}
    try:
        p, derived = build_case(case, device)
    finally:
        os.environ.update(saved)
    out = {}
    for ph in [p.fwd_train, p.fwd_eval, p.bwd, p.opt["adam"]] + derived:
        out[ph.name] = dump_phase(ph)
    counters = {k: int(getattr(p, k, 0) or 0) for k in ("n_folded", "n_dgrad_bnstats", "n_wgrad_merged")}
    meta = {"buckets": getattr(p, "buckets", None), "num_launches": p.num_launches(), "opt_segs": p.opt_segs, **counters}
    out["meta"] = json.dumps(_Canon()(meta), sort_keys=True, indent=0) + "\n"
    return out


def fingerprint(case, device="cpu") -> dict:
    return {k: hashlib.sha256(v.encode()).hexdigest() for k, v in dump_case(case, device).items()}


def _golden(path):
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES)
def test_lowering_fingerprint(case):
    assert fingerprint(case) == _golden(GOLDEN_CPU)[case]


@pytest.mark.gpu
def test_tuned_lowering_fingerprint_gpu():
    """The tuned path (config table, conv workspaces kept per phase) exists only on the device: Model A at batch
    32 through ``autotune_program(measure=False)`` against the hashes recorded on an MI355X."""
    assert fingerprint(GPU_CASE, "cuda") == _golden(GOLDEN_GPU)[GPU_CASE]


def main(argv):
    gpu = "--gpu" in argv
    cases, device, path = ([GPU_CASE], "cuda", GOLDEN_GPU) if gpu else (CASES, "cpu", GOLDEN_CPU)
    if "--out" in argv:  # record somewhere else (e.g. to compare two runs)
        path = argv[argv.index("--out") + 1]
    if "--dump" in argv:
        d = argv[argv.index("--dump") + 1]
        os.makedirs(d, exist_ok=True)
        for case in cases:
            for phase, text in dump_case(case, device).items():
                with open(os.path.join(d, f"{case.replace('/', '_')}.{phase}.txt"), "w") as f:
                    f.write(text)
    if "--write" in argv:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump({case: fingerprint(case, device) for case in cases}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main(sys.argv[1:])

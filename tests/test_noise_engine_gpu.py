"""GPU, engine level: SNR noise in the step's gather phase (StepRunner.set_train_noise / set_eval_noise) on Model B,
the smallest program: batch 4, a 16-sample synthetic set.  The kernel-level reference is ops.functional.
gather_batch_noise, itself tested against the fp64 definition (tests/test_noise_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, SEED, RANGE = 4, 0xABCDEF0123456789, (0.0, 20.0)


@pytest.fixture(scope="module")
def data():
    from mtl_das_pytorch_amd.data.synthetic import generate
    X, d, e = generate(16, seed=0, device="cuda")
    return X, torch.stack([d, e], 1)


def _prog(seed=0):
    from mtl_das_pytorch_amd.engine.mtl import MTLProgram
    from mtl_das_pytorch_amd.models import build_model
    torch.manual_seed(seed)
    prog = MTLProgram(build_model("single_event"), B, "cuda")
    prog.set_optimizer(weight_decay=1e-5)
    return prog


def _runner(prog, data, **kw):
    from mtl_das_pytorch_amd.engine.step import StepRunner
    r = StepRunner(prog, data[0], data[1], **kw)
    r.set_lr(1e-3)
    return r


def _bits(t):
    return t.contiguous().view(torch.int16)


SCHED = torch.tensor([[3, 9, 3, 14], [0, 1, 2, 15], [7, 7, 8, 5]])


def test_step_input_is_the_kernel_reference_at_each_draw(data):
    """With train noise on, the stem's input after step k is the noise gather of schedule row k at draw d0 + k:
    the warm-up and the capture consumed no draws."""
    from mtl_das_pytorch_amd.ops import functional as F
    X, lab = data
    prog = _prog()
    r = _runner(prog, data)
    r.set_index_schedule(SCHED)
    d0 = 5
    r.set_train_noise(RANGE, SEED, draw=d0)
    P = F.sample_power(X)
    snr = torch.tensor(RANGE, dtype=torch.float32).cuda()
    taps, off = prog.stem_pack
    assert taps == 7  # the packed stem
    for k in range(3):
        r.train_step()
        torch.cuda.synchronize()
        want, want_lab = F.gather_batch_noise(X, lab, SCHED[k].cuda(), P, snr, torch.tensor([d0 + k]).cuda(), SEED,
                                              taps=taps, off=off)
        assert torch.equal(_bits(prog.x.view(-1)), _bits(want.view(-1))), k
        assert torch.equal(prog.labels.view(-1), want_lab.view(-1))
        assert r.noise_draw["train"].item() == d0 + k + 1
    assert "train_full" in r.graphs
    r.close()


def test_captured_step_equals_eager_launches(data):
    out = []
    for use_graph in (True, False):
        prog = _prog()
        r = _runner(prog, data, use_graph=use_graph)
        r.set_train_noise(RANGE, SEED, draw=2)
        for k in range(3):
            r.train_step(SCHED[k].cuda())
        torch.cuda.synchronize()
        assert r.noise_draw["train"].item() == 5
        out.append(prog.flat.params.clone())
        r.close()
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("use_graph", [False, True])
def test_determinism_check_with_noise(data, use_graph):
    from mtl_das_pytorch_amd.engine.determinism import check_step
    res = check_step(_prog(), data[0], data[1], SCHED[0].cuda(), use_graph=use_graph, noise=(RANGE, SEED))
    assert res["bitwise_equal"], res


def test_eval_noise_levels_without_recapture(data):
    prog = _prog()
    r = _runner(prog, data, X_eval=data[0], labels_eval=data[1])
    idx = torch.arange(B, device="cuda")

    def metrics():
        r.reset_metrics()
        r.eval_step(idx)
        torch.cuda.synchronize()
        return prog.metrics.clone()

    clean = metrics()
    r.set_eval_noise(20.0)
    m20 = metrics()
    g = r.graphs["eval"]
    assert torch.equal(m20, metrics())  # the same test noise every time
    r.set_eval_noise(-5.0)
    m5 = metrics()
    assert r.graphs["eval"] is g  # another level: device scalars only
    r.set_eval_noise(-5.0, draw=1)
    m5b = metrics()
    assert r.graphs["eval"] is g
    assert not torch.equal(m20, m5) and not torch.equal(m5, m5b) and not torch.equal(clean, m20)
    r.set_eval_noise(None)
    assert "eval" not in r.graphs
    assert torch.equal(metrics(), clean)  # back to the clean gather, bitwise
    # another eval set: its own power table
    X2 = data[0][8:].contiguous()
    r.set_eval_noise(20.0)
    p1 = r._noise_power("eval")
    r.set_eval_source(X2, data[1][8:].contiguous())
    assert r._noise_power("eval") is not p1 and r._noise_power("eval").shape == (8, 1)
    metrics()
    r.close()


def test_noise_off_is_the_step_that_never_heard_of_noise(data):
    from mtl_das_pytorch_amd.engine.program import k_gather
    out = []
    for touched in (False, True):
        prog = _prog()
        r = _runner(prog, data)
        if touched:
            r.set_train_noise(RANGE, SEED)
            r.train_step(SCHED[0].cuda())  # a noisy graph was captured and is dropped again
            r.set_train_noise(None)
            assert not r.graphs
            prog2 = _prog()  # same initial state as the untouched run
            prog.flat.params.copy_(prog2.flat.params)
            for name in ("exp_avg", "exp_avg_sq", "bn_mean", "bn_var", "bn_nbt", "step"):
                getattr(prog.flat, name).copy_(getattr(prog2.flat, name))
            r.pack_weights()
        ph = prog.gather_phase(data[0], data[1], r.idx, clear=True)
        gathers = [l for l in ph.launches if l.name != "clear"]
        assert [(l.name, l.fn) for l in gathers] == [("gather", k_gather)] and "noise" not in gathers[0].d
        for k in range(3):
            r.train_step(SCHED[k].cuda())
        torch.cuda.synchronize()
        out.append(prog.flat.params.clone())
        r.close()
    assert torch.equal(out[0], out[1])


def test_noise_needs_a_resident_source(data):
    r = _runner(_prog(), data, resident=False)
    with pytest.raises(ValueError, match="resident"):
        r.set_train_noise(RANGE, SEED)
    with pytest.raises(ValueError, match="resident"):
        r.set_eval_noise(0.0)
    r.close()


def test_engine_backend_round_trips_the_draw(data):
    from mtl_das_pytorch_amd.engine.backends import EngineBackend
    from mtl_das_pytorch_amd.models import build_model
    from mtl_das_pytorch_amd.parallel.dist import init_distributed
    X, lab = data

    def backend():
        torch.manual_seed(0)
        return EngineBackend(build_model("single_event").cuda(), "single_event", X, lab, X, lab, init_distributed(),
                             batch=B, lr=1e-3, weight_decay=1e-5, noise_snr=RANGE, noise_seed=3)

    be = backend()
    assert be.runner.noise_seed["train"] == 3 and be.runner.noise_snr["train"].tolist() == [0.0, 20.0]
    for k in range(2):
        be.train_batch(SCHED[k].cuda())
    st = be.optimizer_state()
    assert st["noise_draw"] == 2
    be.close()
    be2 = backend()
    assert be2.runner.noise_draw["train"].item() == 0
    be2.load_optimizer_state(st)
    assert be2.runner.noise_draw["train"].item() == 2 and be2.optimizer_state()["noise_draw"] == 2
    be2.close()

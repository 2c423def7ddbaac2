"""Model C (Inception-v3 multi-classifier) as benchmarked -- batch 32, the shipped config table, batched tails and
weight gradients, the normalise-on-load plan of that batch -- layer by layer against tests/layer_ref.py: fp64
references of every single op on the device, at bounds derived from the number formats (layer_ref's docstring), not
the blanket 2e-2 of test_inception_gpu.py::test_inception_backward_layer_local (which keeps its role: B = 8, untuned
configs, cin = 2).

Wiring by teacher forcing.  The torch module itself runs in fp64; every ``BasicConv2d.forward``, the two pool helpers
of models/multi_classifier.py, the stem's ``MaxPool2d`` modules and the classifier (``avgpool`` -> dropout -> ``fc``)
are replaced by one ``torch.autograd.Function`` whose forward receives the input the module's own ``forward`` built
(``torch.cat`` included) from the ENGINE's outputs of the earlier ops, checks it against the engine's input activation
of that op, checks the op, and returns the engine's stored output -- so an error never propagates, and the dataflow
checked is the module's, not one read off the engine's launch records.  Its backward receives the gradient torch's
graph summed from the engine ``dx`` of the consumers, checks it against the sum of ``op.out.grad_sources()``, checks
the op's backward and returns the engine's ``dx``.  Every op could be forced this way, pools and fused heads
included, so every forced input and incoming gradient is compared EXACTLY (a sum of at most six bf16 numbers is exact
in fp64): the engine's source lists are never used to build a reference input.  A fused 1x1 head (``HConv``): each
member checks its own y slice, BN and weight gradient; the joint ``dx`` is checked once against the sum of the
members' fp64 data gradients, the last member to run returns it and the others return zero.  The producer of a
normalise-on-load conv has no stored output: it returns the consumer's operand rebuilt from its stored y and
constants, and the consumer is checked with that operand's rounding-boundary ambiguity (fwd_ref.nol_conv).

Worst observed values on MI355X: docs/ACCURACY.md, "Layer-local checks at the benchmarked batch"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 32


def nhwc(a):
    """A (possibly channel-sliced) engine NHWC activation as dense fp64 [B, H, W, C]."""
    t = a.t.reshape(-1)[a.off:]
    idx = torch.arange(a.M, device=t.device)[:, None] * a.ld + torch.arange(a.C, device=t.device)[None]
    return t[idx].double().view(a.B, a.H, a.W, a.C)


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def to_nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


class _Forced(torch.autograd.Function):
    """One forced op: ``h.fwd`` / ``h.bwd`` check and return the engine's own output / data gradient."""

    @staticmethod
    def forward(ctx, x, h):
        ctx.h = h
        return h.fwd(x.detach())

    @staticmethod
    def backward(ctx, g):
        return ctx.h.bwd(g), None


def table_use(prog):
    """Which launches of the three phases take their config from the shipped table (engine/tune.py applies an entry
    iff the launch's signature is in it), before autotune_program batches them: {(phase, block): [table, heuristic]}
    over the conv and weight-gradient launches (block: "stem" or the Mixed block's index), the totals per launch
    class, and the signatures that fell back to the heuristic."""
    from mtl_das_pytorch_amd.engine.inception import HConv
    from mtl_das_pytorch_amd.engine.tune import conv_signature, load_cache, tail_bwd_signature, wgrad_signature
    cache = load_cache()
    block_of = {}
    for i, op in enumerate(prog.ops):
        if getattr(op, "conv", None) is None:
            continue
        meta = prog.op_meta[prog.ops.index(op.members[0])] if isinstance(op, HConv) else prog.op_meta[i]
        block_of[id(op.conv)] = "stem" if meta is None else meta[0]
    per_block, totals, fallbacks = {}, {}, []
    for ph in (prog.fwd_train, prog.fwd_eval, prog.bwd):
        for l in ph.launches:
            if l.is_conv:
                cls, sig = ("conv_fwd" if l.is_conv_fwd else "conv_dgrad"), conv_signature(l.args[0], l.G, l.d)
                blk = block_of[id(l.owner)]
            elif l.is_wgrad and l.owner is not None:
                cls, sig, blk = "wgrad", wgrad_signature(l.G, l.d), block_of[id(l.owner)]
            elif l.is_tail_bwd and l.d.get("fused") not in (2, 3):
                cls, sig, blk = "tail_bwd", tail_bwd_signature(l.kind, l.G, l.d), None
            else:
                continue
            hit = sig in cache
            totals.setdefault((ph.name, cls), [0, 0])[0 if hit else 1] += 1
            if blk is not None:
                per_block.setdefault((ph.name, blk), [0, 0])[0 if hit else 1] += 1
            if not hit:
                fallbacks.append(sig)
    return per_block, totals, sorted(set(fallbacks))


class Step:
    """The benchmarked program after one training step, and the forced passes over it (each run once)."""

    def __init__(self):
        import layer_ref as L
        from mtl_das_pytorch_amd.data.synthetic import generate
        from mtl_das_pytorch_amd.engine.inception import CBR, InceptionProgram, Pool
        from mtl_das_pytorch_amd.engine.tune import autotune_program
        from mtl_das_pytorch_amd.models import Multi_Classifier, encode_joint
        torch.manual_seed(0)
        self.L = L
        self.model = model = Multi_Classifier(in_channels=1)
        self.prog = prog = InceptionProgram(model, B, "cuda", p_drop=0.5)
        self.use = table_use(prog)
        autotune_program(prog, measure=False)  # as bench.py and test_guard_gpu.py set the program up
        X, d, e = generate(B, seed=11, device="cuda")
        self.labels = encode_joint(d, e)
        self.xq = X.bfloat16().double()
        idx = torch.arange(B, device="cuda")
        prog.opt["pack"].run()
        prog.arena.clear()
        prog.gather_phase(X, self.labels, idx).run()
        prog.fwd_train.run()
        prog.bwd.run()
        torch.cuda.synchronize()
        prog.flat.sync_module_grads()
        self.names = {id(m): n for n, m in model.named_modules()}
        self.cbrs = [op for op in prog.ops if isinstance(op, CBR)]
        self.pools = [op for op in prog.ops if isinstance(op, Pool)]
        self.training = True
        self.fwd_chk = self.bwd_chk = self.eval_chk = None

    # ---- what a tail or a normalise-on-load consumer evaluates
    def consts(self, bn):
        m = bn.mods[0]
        if self.training:
            return bn.consts[0].double()
        return self.L.bn_eval(m.running_mean, m.running_var, m.weight.detach(), m.bias.detach(), bn.eps)

    def operand(self, p):
        """(operand, slack) of the consumer of the normalise-on-load producer ``p``."""
        k = self.consts(p.bn)
        y = nhwc(p.y)
        slack = 0.0 if self.training else self.L.eval_nol_slack(y, k, p.bn.mods[0].bias.detach())
        return y, k, slack

    # ---- the forced passes
    def _force(self, mp):
        from mtl_das_pytorch_amd.models import multi_classifier as mc
        model = self.model
        for op in self.cbrs:
            h = ConvH(self, op)
            mp.setattr(op.module, "forward", lambda x, h=h: _Forced.apply(x, h), raising=False)
        it = iter(self.pools)

        def pool(is_max):
            def run(x):
                op = next(it)
                assert bool(op.is_max) == is_max, "the module's pools and the engine's run in different orders"
                return _Forced.apply(x, PoolH(self, op))
            return run
        mp.setattr(mc, "_avgpool3", pool(False))
        mp.setattr(mc, "_maxpool3s2", pool(True))
        mp.setattr(model.maxpool1, "forward", pool(True), raising=False)
        mp.setattr(model.maxpool2, "forward", pool(True), raising=False)
        head = HeadH(self)
        mp.setattr(model.avgpool, "forward", lambda x: _Forced.apply(x, head), raising=False)
        mp.setattr(model.dropout, "forward", lambda x: x, raising=False)
        mp.setattr(model.fc, "forward", lambda x: x, raising=False)
        return it

    def _run(self, backward):
        L = self.L
        self.hstate = {}
        with pytest.MonkeyPatch.context() as mp, L.on("cuda"):
            it = self._force(mp)
            x = to_nchw(self.xq.permute(0, 2, 3, 1)).requires_grad_(backward)
            with torch.set_grad_enabled(backward):
                out = self.model(x)
            assert next(it, None) is None, "the module ran fewer pools than the engine"
            if backward:
                out.sum().backward()

    def train(self):
        if self.fwd_chk is None:
            assert self.eval_chk is None
            self.training, self.chk, self.bchk = True, self.L.Checker(), self.L.Checker()
            self.metrics, self.confusion = self.prog.metrics.double(), self.prog.confusion.long()
            self._run(True)
            self.fwd_chk, self.bwd_chk = self.chk, self.bchk
        return self

    def eval(self):
        if self.eval_chk is None:
            self.train()  # the eval forward overwrites the activations the training passes read
            prog = self.prog
            met0, cm0 = prog.metrics.double().clone(), prog.confusion.long().clone()
            state = [b.clone() for b in (prog.flat.bn_mean, prog.flat.bn_var, prog.flat.bn_nbt)]
            prog.fwd_eval.run()
            torch.cuda.synchronize()
            self.training, self.chk, self.bchk = False, self.L.Checker(), None
            self.metrics, self.confusion = prog.metrics.double() - met0, prog.confusion.long() - cm0
            now = (prog.flat.bn_mean, prog.flat.bn_var, prog.flat.bn_nbt)
            for name, b, b0 in zip(("mean", "var", "num_batches_tracked"), now, state):
                self.chk.bits(f"running {name} unchanged by the eval forward", b, b0)
            self._run(False)
            self.eval_chk = self.chk
        return self


class ConvH:
    """One BasicConv2d: a CBR op of the engine (its own conv, or a member of a fused head)."""

    def __init__(self, S, op):
        self.S, self.op = S, op
        self.name = S.names[id(op.module)]
        self.hc = op.fused[0] if op.fused is not None else None
        self.n0 = op.fused[1] if op.fused is not None else 0
        self.first = op is S.cbrs[0]

    def _operand(self):
        """The conv's input operand [B, H, W, Cin] in fp64 from the ENGINE's buffers (checked against the forced
        input in ``fwd``); the stem reads the bf16-rounded batch."""
        S, op, L = self.S, self.op, self.S.L
        if self.first:
            return S.xq.permute(0, 2, 3, 1).contiguous()
        if op.nol_from is not None:
            y, k, slack = S.operand(op.nol_from)
            return L.FR.nol_operand(y, k[0], k[1], L.ACT_RELU, slack=slack)[0]
        src = self.hc.src if self.hc is not None else op.src
        return nhwc(src.act)[..., :op.module.conv.in_channels]

    def fwd(self, x):
        S, op, L, chk, nm = self.S, self.op, self.S.L, self.S.chk, self.name
        conv, bn = op.module.conv, op.bn.mods[0]
        xin = to_nhwc(x)
        self.zero_dx = torch.zeros_like(x)
        w = conv.weight.detach()
        if op.nol_from is not None:
            y, k, slack = S.operand(op.nol_from)
            f = L.nol_conv_fwd(y, k[0], k[1], L.ACT_RELU, w, conv.stride, conv.padding, slack=slack)
            chk.true(f"{nm} input is the rebuilt operand", bool(((xin == f["operand"]) | f["amb_map"]).all()))
            chk.true(f"{nm} operand ambiguity below 1 %", float(f["amb_map"].double().mean()) <= 0.01)
            amb = f["amb"]
        else:
            if not self.first:
                chk.exact(f"{nm} input", self._operand(), xin)
            f = L.conv_fwd(xin, w, conv.stride, conv.padding)
            amb = None
        chk.acc("y" if amb is None else "nol y", f"{nm} y", nhwc(op.y), f["y"], f["abs"], f["n"], amb)
        if S.training:
            ref = L.bn_train(f["y"], f["abs"], f["n"], bn.weight.detach(), bn.bias.detach(), op.bn.eps, amb)
            run = (bn.running_mean, bn.running_var, torch.zeros_like(bn.running_mean), torch.ones_like(bn.running_var),
                   bn.num_batches_tracked, 0)
            chk.bn_training(f"{nm} BN", op.bn.consts[0], ref, bn.bias.detach(), run, op.bn.momentum)
        k = S.consts(op.bn)
        if op.skip_tail:  # never materialised: the consumer's operand stands for it
            yk, kk, slack = S.operand(op)
            return to_nchw(L.FR.nol_operand(yk, kk[0], kk[1], L.ACT_RELU, slack=slack)[0])
        out = nhwc(op.out.act)
        chk.ulp("tail", f"{nm} tail", out, L.tail_fwd(L.ACT_RELU, nhwc(op.y), k))
        return to_nchw(out)

    def bwd(self, g):
        S, op, L, chk, nm = self.S, self.op, self.S.L, self.S.bchk, self.name
        conv, bn = op.module.conv, op.bn.mods[0]
        srcs = [nhwc(a) for a in op.out.grad_sources()]
        chk.exact(f"{nm} incoming gradient", sum(srcs), to_nhwc(g))
        o = L.tail_bwd(L.ACT_RELU, nhwc(op.y), op.bn.consts[0], bn.weight.detach(), srcs)
        chk.tail_grads(f"{nm} tail", o, bn.weight.grad, bn.bias.grad, dy=nhwc(op.dy))
        x, dy, w = self._operand(), nhwc(op.dy), conv.weight.detach()
        wg = L.conv_wgrad(x, dy, w.shape, conv.stride, conv.padding)
        chk.l2("dW", f"{nm} dW", conv.weight.grad, wg["dW"])
        holder = self.hc if self.hc is not None else op
        if holder.dx is None:
            return self.zero_dx
        d = L.conv_dgrad(w, dy, x.shape[1:3], conv.stride, conv.padding)
        dx = nhwc(holder.dx)
        if self.hc is None:
            chk.acc("dx", f"{nm} dx", dx, d["g"], d["abs"], d["n"])
            return to_nchw(dx)
        st = S.hstate.setdefault(id(self.hc), {"g": 0.0, "abs": 0.0, "n": 0, "count": 0})
        st["g"], st["abs"], st["n"], st["count"] = st["g"] + d["g"], st["abs"] + d["abs"], st["n"] + d["n"], st["count"] + 1
        if st["count"] < len(self.hc.members):
            return self.zero_dx
        chk.acc("dx", f"{nm} (fused head) joint dx", dx, st["g"], st["abs"], st["n"])
        return to_nchw(dx)


class PoolH:
    def __init__(self, S, op):
        self.S, self.op = S, op
        self.name = ("max" if op.is_max else "avg") + f" pool {S.pools.index(op)}"

    def fwd(self, x):
        S, op, L, chk, nm = self.S, self.op, self.S.L, self.S.chk, self.name
        xin = to_nhwc(x)
        self.zero_dx = torch.zeros_like(x)
        chk.exact(f"{nm} input", nhwc(op.src.act), xin)
        out = nhwc(op.out.act)
        if op.is_max:
            y, am = L.maxpool_fwd(xin)
            chk.exact(f"{nm} y", out, y)
            if S.training and op.am is not None:
                chk.exact(f"{nm} argmax bytes", op.am.view(am.shape).long(), am)
        else:
            chk.ulp("avg pool", f"{nm} y", out, L.avgpool_fwd(xin))
        return to_nchw(out)

    def bwd(self, g):
        S, op, L, chk, nm = self.S, self.op, self.S.L, self.S.bchk, self.name
        srcs = [nhwc(a) for a in op.out.grad_sources()]
        chk.exact(f"{nm} incoming gradient", sum(srcs), to_nhwc(g))
        if op.dx is None:
            return self.zero_dx
        s = op.src.act
        if op.is_max:
            d = L.maxpool_bwd(srcs, L.maxpool_fwd(nhwc(s))[1], s.H, s.W)
        else:
            d = L.avgpool_bwd(srcs)
        dx = nhwc(op.dx)
        chk.acc("max pool dx" if op.is_max else "avg pool dx", f"{nm} dx", dx, d["g"], d["abs"], d["n"])
        return to_nchw(dx)


class HeadH:
    """GAP -> dropout -> fc -> cross entropy (csrc/head.hip cls_head) at test_heads_gpu.py's bounds, given the engine's
    own dropout mask: fc_feat relative 1e-5 on the kept channels, logits relative L2 1e-4, the CE sum relative 1e-4,
    counts and confusion matrices exact (a prediction whose two largest fp64 logits are within 1e-5 is taken from the
    engine's logits), d(logits) atol 1e-6 + rtol 1e-4, the feature gradient relative L2 4e-3 (bit-equal over the
    pixels of a sample), d(fc) from the head's own d(logits) and features relative L2 1e-4."""

    def __init__(self, S):
        self.S = S

    def fwd(self, x):
        S, chk, prog = self.S, self.S.chk, self.S.prog
        xin = to_nhwc(x)
        chk.exact("classifier input", nhwc(prog.feat.act), xin)
        gap = xin.mean((1, 2))
        feat = prog.fc_feat.double()
        p = prog.p_drop if S.training else 0.0
        keep = (feat != 0) | (gap == 0) if S.training else torch.ones_like(gap, dtype=torch.bool)
        if S.training:
            share = float(keep[gap > 0].double().mean())
            chk.true(f"dropout keeps about 1 - p of the channels ({share:.4f})", abs(share - (1 - p)) < 0.01)
        ref = gap * keep / (1.0 - p)
        chk.bounded("fc_feat err / (1e-5 ref)", "fc_feat", feat, ref, 1e-5 * ref.abs())
        fc = S.model.fc
        z = ref @ fc.weight.detach().double().t() + fc.bias.detach().double()
        ze = prog.logp.double()
        chk.l2("logits", "logits", ze, z, 1e-4)
        lab = S.labels
        lp = torch.log_softmax(z, 1)
        ce = -lp[torch.arange(B), lab].sum()
        top = z.topk(2, 1).values
        decided = (top[:, 0] - top[:, 1]) > 1e-5
        pred = torch.where(decided, z.argmax(1), ze.argmax(1))
        chk.exact("decided predictions", ze.argmax(1)[decided], z.argmax(1)[decided])
        ld, le, pd, pe = lab % 16, lab // 16, pred % 16, pred // 16
        nB = torch.tensor(B, device=lab.device)
        zero = torch.zeros((), dtype=torch.int64, device=lab.device)
        chk.bounded("CE sum err / (1e-4 ref)", "CE sum", S.metrics[0, 0], ce, 1e-4 * ce.abs())
        want = torch.stack([torch.stack([(pred == lab).sum(), nB, zero]),
                            torch.stack([(pd == ld).sum(), nB, (pd - ld).abs().sum()]),
                            torch.stack([(pe == le).sum(), nB, zero])])
        chk.exact("metrics: correct, count, |distance error|", S.metrics[:, 1:], want)
        chk.exact("metrics: distance / event loss columns", S.metrics[1:, 0], torch.zeros(2))
        cm = torch.zeros(2, 16, 16, dtype=torch.int64, device=lab.device)
        cm[0].index_put_((ld, pd), torch.ones_like(lab), accumulate=True)
        cm[1].index_put_((le, pe), torch.ones_like(lab), accumulate=True)
        chk.exact("confusion", S.confusion, cm)
        self.z, self.keep, self.p, self.dead = z, keep, p, gap == 0
        return ze[:, :, None, None]

    def bwd(self, g):
        S, chk, prog = self.S, self.S.bchk, self.S.prog
        fc, a = S.model.fc, prog.feat.act
        dl = torch.softmax(self.z, 1)
        dl[torch.arange(B), S.labels] -= 1.0
        dl /= B
        dle = prog.dlogits.double()
        chk.bounded("dlogits err / (1e-6 + 1e-4 ref)", "dlogits", dle, dl, 1e-6 + 1e-4 * dl.abs())
        dfe = nhwc(prog.dfeat)
        # a channel whose GAP is exactly zero (a dead ReLU channel) shows its dropout decision only in the gradient:
        # there the engine's own feature gradient gives the mask (nonzero: kept), which must again be about 1 - p
        keep = torch.where(self.dead, dfe[:, 0, 0] != 0, self.keep)
        if bool(self.dead.any()):
            n, share = int(self.dead.sum()), float(keep[self.dead].double().mean())
            chk.true(f"dropout keeps about 1 - p of the {n} dead channels ({share:.4f})",
                     abs(share - (1 - self.p)) < 5 * (self.p * (1 - self.p) / n) ** 0.5)
        dx = (dl @ fc.weight.detach().double()) * keep / (1.0 - self.p) / (a.H * a.W)
        chk.l2("dhead", "classifier feature gradient", dfe, dx[:, None, None, :].expand_as(dfe), 4e-3)
        chk.exact("feature gradient equal over the pixels", dfe, dfe[:, :1, :1].expand_as(dfe))
        chk.l2("dfc", "fc.weight grad", fc.weight.grad, dle.t() @ prog.fc_feat.double(), 1e-4)
        chk.l2("dfc", "fc.bias grad", fc.bias.grad, dle.sum(0), 1e-4)
        return to_nchw(dfe)


@pytest.fixture(scope="module")
def step():
    # the fp64 references run on PyTorch's native convolutions, not MIOpen (as in test_mtl_layer_local_gpu.py)
    flags = (torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.enabled = False
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield Step()
    torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = flags
    torch.cuda.empty_cache()  # the fp64 references of whole layers: gigabytes the later modules should not inherit


def test_c_program_is_the_benchmarked_one(step):
    """The fixture's program has what only the batch-32, table-configured program has: the normalise-on-load plan of
    that batch, batched forward tails, batched tail backwards, batched weight gradients; the stem and every Mixed
    block run at least one table-configured launch in each phase.

    The plan: a conv above NOL_MAX_PX normalises on load iff its training entry in the shipped table is a patch
    config (``_patch_forward``); that is asserted in both directions for every conv.  With the table as shipped the
    rule selects NO conv: the two candidates' training entries are not patch configs (47x122 3x3 "...|st1": 2, an
    implicit-GEMM config -- only its eval entry "...|st0": 195 is a patch config, and ``_patch_forward`` asks for
    st1; 21x58 3x3: 16, an LDS config), so both keep their BN+ReLU tails at batch 32 and are checked here with a
    materialised input.  What does differ from B = 8: Conv2d_4a_3x3 (21x58, 38,976 output pixels at batch 32) no
    longer normalises on load, as it does at B = 8 (9,744 <= NOL_MAX_PX)."""
    prog = step.prog
    producer = {id(op.out): op for op in step.cbrs}
    for op in step.cbrs:
        if op.conv is None or op.conv.M_out <= prog.NOL_MAX_PX or id(op.src) not in producer:
            continue
        nm = step.names[id(op.module)]
        print(f"{nm}: {op.conv.Ho}x{op.conv.Wo}, {op.conv.M_out} output pixels > NOL_MAX_PX, patch config in the table: "
              f"{prog._patch_forward(op.conv)}, normalises on load: {op.nol_from is not None}")
        assert (op.nol_from is not None) == prog._patch_forward(op.conv), nm
    nol = [op for op in step.cbrs if op.nol_from is not None]
    print(f"{len(nol)} normalise-on-load convs, largest {max(op.conv.M_out for op in nol)} output pixels")
    assert nol and prog.n_nol == len(nol)
    assert step.cbrs[4].module is step.model.Conv2d_4a_3x3 and step.cbrs[4].nol_from is None
    assert prog.n_tail_batched > 0 and any(l.name.startswith("tailbatch") for l in prog.fwd_train.launches)
    assert prog.n_tail_bwd_batched > 0
    assert any(l.is_wgrad_batch for l in prog.bwd.launches)
    per_block, totals, fallbacks = step.use
    for (ph, cls), (hit, miss) in sorted(totals.items()):
        print(f"{ph} {cls}: {hit} from the shipped table, {miss} heuristic")
    print(f"{len(fallbacks)} heuristic signatures:", *fallbacks, sep="\n  ")
    blocks = ["stem"] + list(range(len(step.model.mixed)))
    for ph in ("forward_train", "forward_eval", "backward"):
        for blk in blocks:
            assert per_block.get((ph, blk), [0, 0])[0] > 0, f"no table-configured launch in {ph} of block {blk}"


def test_c_forward_train(step):
    """Per op of ``fwd_train``: the forced input (exact), the pre-BN y (acc bound; a normalise-on-load consumer with its
    operand ambiguity), the published constants against the fp64 statistics of the unrounded reference y, running
    mean / variance and num_batches_tracked, the tail output within one bf16 ulp (a skipped tail: the consumer's
    operand), the pools (max exact, with the argmax bytes; average one ulp), fc_feat / logits / metrics."""
    step.train().fwd_chk.done()


def test_c_backward(step):
    """Per op of ``bwd``: the incoming gradient torch's graph summed against the engine's sources (exact), the tail
    backward (dy relative L2 6e-3, d(gamma) / d(beta) 1e-5 and the per-channel sums rule with the mask-ambiguous
    elements by their |term|), dW (2e-4), dx (acc bound; a fused head's joint dx once), the pool gradients (acc bound)
    and the classifier's d(logits), feature gradient and fc gradients."""
    step.train().bwd_chk.done()


def test_c_forward_eval(step):
    """``fwd_eval`` (the ``st0`` configs) on the same batch after the step moved the running statistics: the same
    checks with the eval constants, no dropout, the running statistics bit-unchanged."""
    step.eval().eval_chk.done()

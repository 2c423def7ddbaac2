"""GPU, kernel level: the batch gather (csrc/misc.hip gather_batch_kernel) in its unpacked channel form -- taps = 0,
Cin real channels zero-padded to 8 -- against its definition (tests/test_noise_gpu.py ``layout`` of the gathered rows,
rounded once to bf16).  The packed-tap form is covered by tests/test_wpath_gpu.py part D.

7 x 10 images, 5 dataset rows, a batch of 3 with a repeated row; index form and schedule form ([nrows = 2][B] table,
cursor 3, row 0 of the table pointing at the poisoned rows).  Dataset rows and labels the launch may not read are
NaN / -777; the output and the labels are followed by sentinels; one 32-float zero range lies inside a 40-float buffer.
"""
import pytest
import torch

from fwd_ref import bf16_rne
from test_noise_gpu import layout

pytestmark = pytest.mark.gpu

SENT = -12288.0  # (exact in bf16, fp32 and int64)
H, W, N, ROWS = 7, 10, 5, (4, 1, 4)


def _lib():
    from mtl_das_pytorch_amd.ops.hip import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


class Gather:
    def __init__(self, Cin):
        g = torch.Generator().manual_seed(40 + Cin)
        self.Cin, self.B = Cin, len(ROWS)
        self.X = 100.0 * torch.randn(N, Cin, H, W, generator=g) + 30.0
        self.unused = [r for r in range(N) if r not in ROWS]
        Xp = self.X.clone()
        Xp[self.unused] = float("nan")
        self.lab = torch.arange(2 * N).view(N, 2) + 100
        labp = self.lab.clone()
        labp[self.unused] = -777
        self.dX, self.dlab = Xp.cuda(), labp.cuda()
        self.n_out = self.B * H * W * 8
        self.out = torch.full((self.n_out + 64,), SENT, dtype=torch.bfloat16, device="cuda")
        self.lab_out = torch.full((self.B * 2 + 16,), int(SENT), dtype=torch.int64, device="cuda")
        self.zero = torch.full((40,), 7.0, device="cuda")

    def args(self, sched):
        """The launch dict (ops.functional.gather_args), writing this case's sentinel-followed buffers."""
        from mtl_das_pytorch_amd.ops.functional import gather_args
        if sched:
            other = (self.unused * self.B)[:self.B]
            self.idx = torch.tensor([other, list(ROWS)]).cuda()
            self.cursor = torch.tensor([3]).cuda()
        else:
            self.idx, self.cursor = torch.tensor(ROWS).cuda(), None
        return gather_args(X=self.dX, labels=self.dlab, lab_w=2, idx=self.idx, out=self.out, lab_out=self.lab_out,
                           B=self.B, H=H, W=W, taps=0, off=0, zero=[(self.zero.data_ptr() + 16, 32 * 4)],
                           cursor=self.cursor)


@pytest.mark.parametrize("sched", [False, True], ids=["index", "schedule"])
@pytest.mark.parametrize("Cin", [2, 3, 8])
def test_unpacked_gather(Cin, sched):
    c = Gather(Cin)
    d = c.args(sched)
    assert d["nrows"] == (2 if sched else 0) and "noise" not in d
    _lib().gather_batch(_stream(), d)
    torch.cuda.synchronize()
    got = c.out[:c.n_out].view(c.B, H, W, 8).cpu()
    want = bf16_rne(layout(c.X[list(ROWS)].double(), 0, 0)).float().bfloat16()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(_bits(got), _bits(want))
    assert (_bits(got[..., Cin:]) == 0).all()            # padding channels: exactly +0
    assert torch.equal(_bits(got[0]), _bits(got[2]))      # the repeated row
    assert (c.out[c.n_out:].float() == SENT).all()
    lab = c.lab_out.cpu()
    assert torch.equal(lab[:c.B * 2].view(c.B, 2), c.lab[list(ROWS)]) and (lab[c.B * 2:] == int(SENT)).all()
    z = c.zero.cpu()
    assert (z[4:36] == 0).all() and (z[:4] == 7).all() and (z[36:] == 7).all()  # only the zero range is cleared
    if sched:
        assert c.cursor.item() == 3                       # the gather reads the cursor, the optimizer advances it
    # the functional layer builds the same launch
    from mtl_das_pytorch_amd.ops import functional as F
    o2, l2 = F.gather_batch(c.dX, c.dlab, c.idx, cursor=c.cursor)
    assert torch.equal(_bits(o2.cpu()), _bits(got)) and torch.equal(l2.cpu(), c.lab[list(ROWS)])


def test_gather_refusals():
    """Each of these is refused by host code before any launch: csrc/stem_gather.h gather_args_ok (rc = -2: Cin > 8,
    taps with Cin != 1, a null output, an empty batch) and the binding (zero ranges, a cursor without its row
    count)."""
    c = Gather(2)
    d = c.args(True)
    z = c.zero.data_ptr()
    bad = [
        ({"Cin": 9}, "rc=-2"),
        ({"Cin": 2, "taps": 3, "off": 1}, "rc=-2"),
        ({"zero": [(z + 4, 32 * 4)]}, "zero range not 16-byte aligned"),
        ({"zero": [(z, 30)]}, "zero range not 16-byte aligned"),
        ({"zero": [(z, 16)] * 5}, "at most 4 zero ranges"),
        ({"nrows": 0}, "row count"),
        ({"out": 0}, "rc=-2"),
        ({"lab_out": 0}, "rc=-2"),
        ({"B": 0}, "rc=-2"),
    ]
    for k, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            _lib().gather_batch(_stream(), {**d, **k})
    torch.cuda.synchronize()
    assert (c.out.float() == SENT).all() and (c.zero == 7).all() and (c.lab_out == int(SENT)).all()

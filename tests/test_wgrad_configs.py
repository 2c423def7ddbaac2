"""The extension's weight-gradient config table and host argument check against their Python copies, on the CPU (the
extension builds and loads without a GPU; no kernel is launched and no pointer is read).

* csrc/wgrad_tile.h WGRAD_CONFIGS (binding ``wgrad_configs``) == ops/functional.py WGRAD_CONFIGS, row by row.
* csrc/conv.hip wgrad_ntiles (binding ``wgrad_ntiles``) == ops/functional.py wgrad_ntiles, which ConvLayer.wgrad_valid
  uses, for every case of wpath_ref.WCASES and for synthetic convs one value on each side of every bound the kernels'
  bit fields and 32-bit offsets set, under all 48 configs.
* Every constant the bindings export that has a Python copy equals it (FIN_EPT has none: engine/core.py reads it
  from the extension)."""
import pytest

import wpath_ref as R
from mtl_das_pytorch_amd.ops import functional as fn
from mtl_das_pytorch_amd.ops.hip import lib

IDS = list(range(0, 20)) + list(range(32, 48))


def test_config_table_matches():
    rows = lib().wgrad_configs()
    assert [r[0] for r in rows] == IDS and sorted(fn.WGRAD_CONFIGS) == IDS
    for cfg, fam, *shape in rows:
        c = fn.WGRAD_CONFIGS[cfg]
        assert (fn.WGRAD_FAMILIES[fam],) + tuple(shape) == tuple(c), cfg
    # the names derived from the table, and the twin relation, as the tools and tests use them
    assert sorted({**fn.WGRAD_TILES, **fn.WGRAD_PATCH}) == IDS and sorted(fn.WGRAD_PATCH) == list(range(12, 20))
    assert all(fn.WGRAD_TILES[c] == tuple(fn.WGRAD_CONFIGS[c][1:4]) for c in fn.WGRAD_TILES)
    assert all(fn.WGRAD_PATCH[c] == (v.TN, v.CB, v.W8, v.R) for c, v in fn.WGRAD_CONFIGS.items() if v.family == "patch")
    for c in IDS:
        t = fn.wgrad_lean_twin(c)
        if fn.wgrad_family(c) == "big":
            assert fn.wgrad_family(t) == "leanbig" and fn.WGRAD_TILES[t] == fn.WGRAD_TILES[c]
        else:
            assert t == c
    assert fn.wgrad_ntiles(20, _geom()) == lib().wgrad_ntiles(20, _geom()) == -1  # no such config


def _geom(B=1, H=4, W=4, C0=8, Co=8, KH=1, KW=1, sh=1, sw=1, ph=0, pw=0, C1=0, ld0=0, ld1=0, ldd=0, Ho=None, Wo=None):
    """The argument dict of a weight-gradient launch, geometry and pitches only (every pointer null)."""
    Cs = C0 + C1
    Ho = (H + 2 * ph - KH) // sh + 1 if Ho is None else Ho
    Wo = (W + 2 * pw - KW) // sw + 1 if Wo is None else Wo
    src = {"ld0": ld0 or C0, "C0": C0, "C1": C1}
    if C1:
        src["ld1"] = ld1 or C1
    return {"src": src, "ldd": ldd or Co, "splits": 1, "m_per_split": B * Ho * Wo, "B": B, "Hi": H, "Wi": W, "Ho": Ho,
            "Wo": Wo, "Co": Co, "Npad": R.pad_to(Co, 16), "Cs": Cs, "KH": KH, "KW": KW, "sh": sh, "sw": sw, "ph": ph,
            "pw": pw, "Kpad": R.pad_to(KH * KW * Cs, 64)}


def _of_case(c):
    return _geom(c.B, c.H, c.W, c.C0, c.Co, c.KH, c.KW, c.sh, c.sw, c.ph, c.pw, c.C1, c.ld0, c.ld1, c.ldd)


IM2COL = ("small", "whole", "big", "lean", "leanbig")
LEAN = ("lean", "leanbig")
# (name, last value inside the bound, first value outside, the families the bound binds).  The bounds:
# * encode_kg (csrc/conv_tile.h): the channel offset within a segment, at most width - 8, in 14 bits -> segments of
#   at most 2^14 channels; the tap indices kh <= KH - 1, kw <= KW - 1 in 7 bits -> KH, KW <= 128;
# * wgrad_lean_block: taps added as 7-bit fields with KH, KW < 128 (its earlier limit, kept); the dy channel
#   n0 + 8 * cg <= (row tiles x TN) - 8 in 14 bits -> Npad padded to the row tile at most 2^14 (TN | 2^14 for
#   every lean tile, so Npad = 2^14 passes and 2^14 + 16 fails under each); fdiv24: M < 2^24; 32-bit offsets:
#   input pixels x pitch and M x dy pitch below 2^31; the pixel table's 16-bit column and row: Wi < 2^15, Hi < 2^14.
BOUNDS = [
    ("segment 0 width", _geom(C0=1 << 14), _geom(C0=(1 << 14) + 8), IM2COL),
    ("segment 1 width", _geom(C0=128, C1=1 << 14), _geom(C0=128, C1=(1 << 14) + 8), IM2COL),
    ("KH field", _geom(H=128, KH=128), _geom(H=129, KH=129), ("small", "whole", "big")),
    ("KW field", _geom(W=128, KW=128), _geom(W=129, KW=129), ("small", "whole", "big")),
    ("lean KH", _geom(H=127, KH=127), _geom(H=128, KH=128), LEAN),
    ("lean KW", _geom(W=127, KW=127), _geom(W=128, KW=128), LEAN),
    ("lean dy channel", _geom(Co=1 << 14), _geom(Co=(1 << 14) + 16), LEAN),
    ("lean M", _geom(H=4097, W=4095), _geom(H=4096, W=4096), LEAN),                  # M = 2^24 - 1, 2^24
    ("lean input offset", _geom(H=1 << 13, W=(1 << 14) - 1, Ho=1, Wo=1, ld0=16),
     _geom(H=1 << 13, W=1 << 14, Ho=1, Wo=1, ld0=16), LEAN),
    ("lean dy offset", _geom(H=2047, W=4096, ldd=256), _geom(H=2048, W=4096, ldd=256), LEAN),
    ("lean Wi", _geom(H=1, W=(1 << 15) - 1), _geom(H=1, W=1 << 15), LEAN),
    ("lean Hi", _geom(H=(1 << 14) - 1, W=1), _geom(H=1 << 14, W=1), LEAN),
]


def test_bound_cases_sit_on_their_bounds():
    """Each pair differs from the bound by one step of the value (8 channels, one tap, one pixel row...)."""
    v = {n: (a, b) for n, a, b, _ in BOUNDS}
    assert v["lean M"][0]["B"] * v["lean M"][0]["Ho"] * v["lean M"][0]["Wo"] < 1 << 24 == v["lean M"][1]["Ho"] * v["lean M"][1]["Wo"]
    a, b = v["lean input offset"]
    assert a["Hi"] * a["Wi"] * a["src"]["ld0"] < 1 << 31 == b["Hi"] * b["Wi"] * b["src"]["ld0"]
    a, b = v["lean dy offset"]
    assert a["Ho"] * a["Wo"] * a["ldd"] < 1 << 31 == b["Ho"] * b["Wo"] * b["ldd"] and b["Ho"] * b["Wo"] < 1 << 24


def test_validity_and_tile_counts_agree():
    L = lib()
    cases = [(c.name, _of_case(c), None, None) for c in R.WCASES]
    for name, inside, outside, fams in BOUNDS:
        cases += [(name + " inside", inside, True, fams), (name + " outside", outside, False, fams)]
    accepted, refused = set(), set()
    for name, d, expect, fams in cases:
        for cfg in IDS:
            fam = fn.wgrad_family(cfg)
            nt, py = L.wgrad_ntiles(cfg, d), fn.wgrad_ntiles(cfg, d)
            assert nt == py, (name, cfg, nt, py)
            assert nt == -2 or nt > 0, (name, cfg, nt)
            (accepted if nt > 0 else refused).add(fam)
            if expect is False and fam in fams:
                assert nt == -2, (name, cfg, nt)
            if expect is True and fam in fams and fam not in ("small", "whole"):  # (their K tiles must divide Kpad)
                assert nt > 0, (name, cfg, nt)
        if expect is True:  # the bound itself refuses nothing: every exact-K-tile family has a config that takes it
            for fam in set(fams) & {"small", "whole"}:
                assert any(L.wgrad_ntiles(c, d) > 0 for c in IDS if fn.wgrad_family(c) == fam), (name, fam)
    assert accepted == refused == set(fn.WGRAD_FAMILIES)


def test_wcases_alone_refuse_only_by_tiling():
    """What the kernel tests launch is not touched by the bounds: a WCASES pair is refused only where its K tiles do
    not divide Kpad (small, whole) or the patch rules say so."""
    for c in R.WCASES:
        for cfg in IDS:
            if fn.wgrad_family(cfg) != "patch":
                assert (fn.wgrad_ntiles(cfg, _of_case(c)) > 0) == (fn.wgrad_ktiles(cfg, c.Kpad) > 0), (c.name, cfg)


CONSTANTS = ["CONV_LDS_CFG0", "CONV_LDS_NCFG", "CONV_DEEP_CFG0", "CONV_DEEP_NCFG", "CONV_GLDS_CFG0", "CONV_GLDS_NCFG",
             "CONV_PATCH_CFG0", "CONV_PATCH_NCFG", "CONV_GDEEP_CFG0", "CONV_GDEEP_NCFG", "CONV_PATCHP_CFG0",
             "CONV_PATCHP_NCFG", "CONV_XCD", "NREP", "DECIMATE_TILE"]


@pytest.mark.parametrize("name", CONSTANTS)
def test_exported_constants_match(name):
    assert getattr(lib(), name) == getattr(fn, name)


def test_one_nrep():
    from mtl_das_pytorch_amd.engine import core
    assert core.NREP is fn.NREP and lib().FIN_EPT > 0

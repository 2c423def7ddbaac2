"""What the activity-gate tests (test_gate.py, test_gate_gpu.py) share: the fixture recording, its windows' fp64
powers (computed once) and the gate's flags written out in fp64, with each window's distance from the threshold."""
import functools

import numpy as np

STRIDE = (10, 50)
GATE_DB = 3.0


@functools.lru_cache(maxsize=None)
def fixture():
    """(rec [230, 700] fp32, fs, ts, power fp64 [140]): unit noise with a 4x louder corner, rows 100.. x times 450..;
    stride (10, 50) gives 14 x 10 windows."""
    from mtl_das_pytorch_amd.inference import WINDOW, window_power_reference, window_starts
    rec = np.random.default_rng(7).standard_normal((230, 700)).astype(np.float32)
    rec[100:230, 450:700] *= 4
    fs, ts = window_starts(230, WINDOW[0], STRIDE[0]), window_starts(700, WINDOW[1], STRIDE[1])
    assert len(fs) == 14 and len(ts) == 10
    power = window_power_reference(rec, fs, ts, WINDOW)
    for a in (rec, power):
        a.setflags(write=False)  # shared: nobody changes it
    return rec, fs, ts, power


def lower_median(power, nt):
    """Per fiber start a: sorted(power[a, :])[(nt - 1) // 2], in plain Python."""
    return np.asarray([sorted(row.tolist())[(nt - 1) // 2] for row in np.asarray(power).reshape(-1, nt)])


def flags(power, nt, gate_db, noise_floor):
    """(active [N] bool, margin_db [N]): the gate in fp64 and every window's distance from its threshold in dB."""
    floor = lower_median(power, nt) if noise_floor == "auto" else np.full(len(power) // nt, float(noise_floor))
    thr = np.repeat(floor, nt) * 10.0 ** (gate_db / 10.0)
    return ~(power < thr), np.abs(10.0 * np.log10(power / thr))


def fixture_flags(noise_floor):
    """The fixture's flags at GATE_DB, after the two conditions that make them a fair test: no window within 0.01 dB
    of the threshold (fp32 rounding, about 1e-6 dB, cannot flip a flag) and an active share of 20 % .. 80 %."""
    _, _, ts, power = fixture()
    active, margin = flags(power, len(ts), GATE_DB, noise_floor)
    print(f"noise_floor={noise_floor}: {int(active.sum())} of {len(active)} active, nearest {margin.min():.3f} dB")
    assert margin.min() > 0.01, margin.min()
    assert 0.2 <= active.mean() <= 0.8, active.mean()
    return active

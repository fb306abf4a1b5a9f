"""CPU: engine.trainer.WarmupSchedule against tests/schedule_ref.py (the reference trainer's loop restated, engine/trainer.py:216-219,305-306,
330,370-380,397-399) and against a table computed from those lines by hand."""
import types

import pytest

import schedule_ref
from improving_yolov8_cbam_swinblock_amd.engine.trainer import WarmupSchedule

TABLE = dict(epochs=12, nb=10, batch=16, nbs=64, lr0=0.01, lrf=0.01, momentum=0.937, weight_decay=5e-4)


def walk(s):
    return [s.advance(s.at(epoch, i)) for epoch in range(s.epochs) for i in range(s.nb)]


@pytest.mark.parametrize("kw", [
    TABLE,
    dict(TABLE, batch=24),
    dict(TABLE, batch=32, cos_lr=True),
    dict(TABLE, batch=128),                                   # nbs / batch < 1: accumulate stays 1
    dict(epochs=3, nb=150, batch=16, warmup_epochs=3.0),      # nw = 450: the warm-up spans the whole run
    dict(epochs=4, nb=60, batch=8, nbs=64, warmup_epochs=0),  # no warm-up: nw = -1
    dict(epochs=2, nb=6, batch=2, nbs=8, warmup_epochs=0.5),
    dict(epochs=5, nb=40, batch=20, nbs=50, warmup_epochs=1.0, warmup_bias_lr=0.0, lr0=0.002, lrf=0.1),  # nbs / batch = 2.5
])
def test_schedule_matches_the_restated_reference_loop(kw):
    s = WarmupSchedule(**kw)
    nw, decay, rows = schedule_ref.run(**kw)
    assert s.nw == nw and s.weight_decay == decay
    got = walk(s)
    assert len(got) == len(rows)
    for g, r in zip(got, rows):
        assert (g.ni, g.accumulate, g.update) == (r["ni"], r["accumulate"], r["update"]), (g, r)
        assert g.lrs == pytest.approx(r["lrs"], rel=0, abs=1e-15) and g.momentum == pytest.approx(r["momentum"], rel=0, abs=1e-15), (g, r)


def test_schedule_table_batch_16():
    s = WarmupSchedule(**TABLE)
    assert s.nw == 100 and s.weight_decay == pytest.approx(5e-4, abs=1e-18)
    rows = walk(s)
    assert len(rows) == 120
    changes = [(r.ni, r.accumulate) for k, r in enumerate(rows) if k == 0 or r.accumulate != rows[k - 1].accumulate]
    assert changes == [(0, 1), (17, 2), (51, 3), (84, 4)]
    assert rows[50].accumulate == 2  # the interpolant is exactly 2.5: halves round to even
    upd = [r.ni for r in rows if r.update]
    assert len(upd) == 54
    assert upd[:17] == list(range(17)) and upd[17:20] == [18, 20, 22]
    assert upd[-8:] == [91, 95, 99, 103, 107, 111, 115, 119]
    near = lambda v: pytest.approx(v, rel=0, abs=1e-12)  # noqa: E731
    assert rows[0].lrs == near([0.1, 0.0, 0.0]) and rows[0].momentum == near(0.8)
    assert rows[50].lrs == near([0.0529375, 0.0029375, 0.0029375]) and rows[50].momentum == near(0.8685)
    for ni in (100, 101):
        assert rows[ni].lrs == near([0.00175] * 3) and rows[ni].momentum == near(0.937)
    assert rows[119].lrs == near([0.000925] * 3)


def test_schedule_table_batch_24():
    s = WarmupSchedule(**dict(TABLE, batch=24))
    assert s.weight_decay == pytest.approx(5.625e-4, abs=1e-18)
    rows = walk(s)
    changes = [(r.ni, r.accumulate) for k, r in enumerate(rows) if k == 0 or r.accumulate != rows[k - 1].accumulate]
    assert changes == [(0, 1), (30, 2), (91, 3)]
    assert sum(r.update for r in rows) == 70


def test_apply_writes_param_groups_and_keeps_the_adam_family_rule():
    """apply() writes lr per group, the momentum only where a group has one (reference :379), the scaled decay into the decayed group; for
    the Adam family the bias group warms up from 0 (:816) and `betas` are left alone."""
    sgd = types.SimpleNamespace(param_groups=[{"lr": 0.01, "momentum": 0.937, "weight_decay": wd} for wd in (0.0, 5e-4, 0.0)])
    adam = types.SimpleNamespace(param_groups=[{"lr": 0.01, "betas": (0.9, 0.999), "weight_decay": wd} for wd in (0.0, 5e-4, 0.0)])
    kw = dict(TABLE, batch=24)
    a, b = WarmupSchedule(**kw), WarmupSchedule(**kw)
    _, _, rows = schedule_ref.run(**kw)
    _, _, rows0 = schedule_ref.run(**dict(kw, warmup_bias_lr=0.0), has_momentum=False)
    for epoch in range(2):
        for i in range(10):
            ra, rb = a.apply(sgd, epoch, i), b.apply(adam, epoch, i)
            ni = epoch * 10 + i
            assert [g["lr"] for g in sgd.param_groups] == pytest.approx(rows[ni]["lrs"], rel=0, abs=1e-15)
            assert all(g["momentum"] == pytest.approx(rows[ni]["momentum"], abs=1e-15) for g in sgd.param_groups)
            assert [g["lr"] for g in adam.param_groups] == pytest.approx(rows0[ni]["lrs"], rel=0, abs=1e-15)
            assert all(g["betas"] == (0.9, 0.999) and "momentum" not in g for g in adam.param_groups)
            assert ra.update == rows[ni]["update"] == rb.update
    assert [g["weight_decay"] for g in sgd.param_groups] == [0.0, pytest.approx(5.625e-4), 0.0]

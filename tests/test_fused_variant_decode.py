"""CPU: _native.fused_variant decodes plgpu_groupby_info.fused_variant's bit
layout (include/polaroid_gpu.h; written by launch_fast_rows)."""

from polaroid_amd import _native as N


def _pack(var, pack, nulls, runs, deriv, limbs, nacc, pred, sumonly, rows, vwords=0):
    return (var | pack << 3 | nulls << 5 | runs << 6 | deriv << 7 | limbs << 8 | nacc << 10 | pred << 13 |
            sumonly << 14 | 1 << 15 | rows << 16 | vwords << 20)


def test_decode_round_trip():
    # the benchmark's variant: gb_fast_kernel<4, 1, true, 2, 2, false, false, false, 5, 1>
    want = dict(var=5, pack=1, nulls=False, runs=False, deriv=False, limbs=2, nacc=4, pred=1, sumonly=True, rows=2,
                ran=True, vwords=False)
    assert N.fused_variant(_pack(5, 1, 0, 0, 0, 2, 4, 1, 1, 2)) == want
    # a NULLS instantiation with whole-word validity reads (bit 20)
    assert N.fused_variant(_pack(0, 0, 1, 0, 0, 2, 2, 1, 1, 2, 1)) == dict(
        var=0, pack=0, nulls=True, runs=False, deriv=False, limbs=2, nacc=2, pred=1, sumonly=True, rows=2, ran=True,
        vwords=True)
    # every field at its largest value, one at a time: no field bleeds into a neighbour
    tops = dict(var=7, pack=3, nulls=1, runs=1, deriv=1, limbs=3, nacc=7, pred=1, sumonly=1, rows=15, vwords=1)
    for name, top in tops.items():
        got = N.fused_variant(_pack(**{**dict.fromkeys(tops, 0), name: top}))
        assert got.pop("ran") is True
        assert got == {k: (type(got[k])(top) if k == name else type(got[k])(0)) for k in tops}, name


def test_decode_sources():
    """The raw value, the info dict of collect(info=...), and the struct; 0
    (the fused kernel did not run) is distinct from <0, 0, false, ...>."""
    gi = N.GroupByInfo()
    assert N.fused_variant(gi) == N.fused_variant({"fused_variant": 0}) == N.fused_variant(0)
    assert N.fused_variant(0)["ran"] is False
    gi.fused_variant = 1 << 15
    assert N.fused_variant(gi)["ran"] is True and N.fused_variant(gi)["nacc"] == 0
    assert "fused_variant" in gi.as_dict() and list(gi.as_dict())[-1] == "_reserved"

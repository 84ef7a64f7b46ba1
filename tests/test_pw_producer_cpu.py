"""The launch lists with the producer fold (engine.Builder.pw_units, _DeferredNorm), built on the CPU: which units lose their
normalise pass and their backward reduction under VT_PW_FOLD_MIN_MB=0, and that nothing changes where the fold does not
apply."""
import torch

from vision_toolbox import _native as N
from vision_toolbox import backbones


def _dry_program(name, dtype=N.VT_BF16, size=64, batch=2):
    m = getattr(backbones, name)()
    m.train(True)
    r = m._vt_runner()
    r.store.ensure(torch.device("cpu"))
    return r.program(torch.zeros(batch, 3, size, size), dtype, True, True)


def _ops(p):
    return ([p.fwd_ops[i] for i in range(p.n_fwd)], [p.bwd_ops[i] for i in range(p.n_bwd)])


def _kind(op):
    return N.OP_NAMES.get(op.kind & 0xFFFF)


def test_stage0_pair_takes_over_the_normalise_pass_and_the_reduction(monkeypatch):
    base = _dry_program("cspdarknet53")  # (the fold's own threshold at its default: these toy tensors stay below it)
    monkeypatch.setenv("VT_PW_FOLD_MIN_MB", "0")
    p = _dry_program("cspdarknet53")
    h0, h = base.kind_histogram, p.kind_histogram
    # the units that open CSP stages 0 and 1 hand their output to conv1 | conv2: the 64 -> 32 | 32 pair keeps its filter
    # gradient in the kernel (mode 2) and folds, the 128 -> 64 | 64 pair (mode 1) needs the stored tensor and does not;
    # stages 2-4 have no pointwise pair
    assert h["bn_fin_apply"] == h0["bn_fin_apply"] - 1
    assert h["bn_bwd_reduce"] == h0["bn_bwd_reduce"] - 1
    assert all(h[k] == h0[k] for k in h0 if k not in ("bn_fin_apply", "bn_bwd_reduce")) and set(h) == set(h0)
    assert p.n_units == base.n_units == 67
    assert p.arena_bytes < base.arena_bytes  # the folded unit's output tensor does not exist
    fwd, bwd = _ops(p)
    folded = [op for op in fwd + bwd if _kind(op) in ("pw_stats", "pw_apply", "pw_apply_fin", "pw_reduce", "pw_bwd", "pw_bwd_fin")
              and op.ptr[20].base >= 0]
    assert [_kind(op) for op in folded] == ["pw_stats", "pw_apply_fin", "pw_reduce", "pw_bwd_fin"]
    for op in folded:
        assert (op.i[0], op.i[1], op.i[3], op.i[4], op.i[20]) == (64, 2, 32, 32, 1)  # K, groups, C0, C1, producer ReLU
    st = folded[0]
    assert all(st.ptr[k].base >= 0 for k in range(5, 11)) and st.f[1] == st.f[0] and st.f[2] > 0  # the producer's finalize
    assert folded[3].ptr[21].base >= 0  # ... and its backward sums, which its bn_bwd_fin_apply then reads
    sums = (folded[3].ptr[21].base, folded[3].ptr[21].offset)
    readers = [op for op in bwd if _kind(op) == "bn_bwd_fin_apply" and (op.ptr[0].base, op.ptr[0].offset) == sums]
    assert len(readers) == 1 and bwd.index(readers[0]) > bwd.index(folded[3])
    # the stage-1 unit keeps its normalise pass: the mode-1 pair reads a stored tensor
    pair1 = [op for op in fwd if _kind(op) == "pw_stats" and op.i[0] == 128 and op.i[1] == 2]
    assert len(pair1) == 1 and pair1[0].ptr[20].base < 0


def test_the_reduction_stays_a_pass_of_its_own_when_asked(monkeypatch):
    base = _dry_program("cspdarknet53").kind_histogram
    monkeypatch.setenv("VT_PW_FOLD_MIN_MB", "0")
    monkeypatch.setenv("VT_PW_FOLD_BNRED", "0")
    h = _dry_program("cspdarknet53").kind_histogram
    assert h["bn_fin_apply"] == base["bn_fin_apply"] - 1 and h["bn_bwd_reduce"] == base["bn_bwd_reduce"]


def test_programs_without_a_qualifying_pair_are_unchanged(monkeypatch):
    """Darknet-53: the stride-2 unit's output is also the first block's shortcut, and nothing asks for a deferral; f32,
    deterministic mode and SyncBatchNorm-free CSPDarknet-53 below the threshold: today's programs byte for byte."""
    def lists(name, dtype=N.VT_BF16):
        p = _dry_program(name, dtype)
        return bytes(p.fwd_ops), bytes(p.bwd_ops), p.arena_bytes

    base = {k: lists(*k) for k in (("darknet53",), ("cspdarknet53", N.VT_F32), ("vovnet39",))}
    monkeypatch.setenv("VT_DETERMINISTIC", "1")
    det = lists("cspdarknet53")
    monkeypatch.setenv("VT_PW_FOLD_MIN_MB", "0")
    assert lists("cspdarknet53") == det
    monkeypatch.delenv("VT_DETERMINISTIC")
    for k, v in base.items():
        assert lists(*k) == v, k
    monkeypatch.setenv("VT_PW_FOLD_MIN_MB", "1e9")
    off = lists("cspdarknet53")
    monkeypatch.delenv("VT_PW_FOLD_MIN_MB")
    assert lists("cspdarknet53") == off

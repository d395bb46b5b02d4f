"""tests/extend_ragged_ref.py without a GPU: the ragged reference is the uniform one per sequence, a guarded sequence has no output
and keeps its caches, and the GPU test's inputs tell a kernel that uses one P for the whole batch from the right one."""
import pytest
import torch

import decode_ref as DR
import extend_ragged_ref as RR
import extend_ref as ER

HEADS, TMAX = 2, 288
BOUND = 2e-5                                                # what tests/test_attention_extend_ragged_gpu.py holds the fp32 kernel to


@pytest.mark.parametrize("positions,Tn", [((0, 63, 200), 1), ((5, 127, 128), 33), ((100, 0, 17), 188)])
def test_the_reference_is_the_uniform_reference_of_every_sequence(positions, Tn):
    qkv, kc, vc = RR.random_extend_ragged(HEADS, TMAX, positions, Tn, torch.float32, seed=7)
    out, k2, v2 = RR.extend_ragged_attention_ref(qkv, kc, vc, positions, True)
    assert out.dtype == torch.float64 and bool(torch.isfinite(out).all())
    for b, P in enumerate(positions):
        assert bool(torch.isnan(kc[b, :, P:]).all()) and bool(torch.isfinite(kc[b, :, :P]).all())
        o, kb, vb = ER.extend_attention_ref(*RR.sequence(qkv, kc, vc, b, Tn), P, True)
        assert torch.equal(out[b * Tn:(b + 1) * Tn], o)
        assert torch.equal(DR.bits(k2[b:b + 1]), DR.bits(kb)) and torch.equal(DR.bits(v2[b:b + 1]), DR.bits(vb))
        assert bool(torch.isnan(k2[b, :, P + Tn:]).all()) and bool(torch.isfinite(k2[b, :, :P + Tn]).all())


def test_a_guarded_sequence_has_no_output_and_keeps_its_caches():
    for positions, Tn in (((5, -1, 128), 33), ((63, 64, TMAX + 1 - 64), 64)):
        bad = [RR.guarded(P, Tn, TMAX) for P in positions]
        assert sum(bad) == 1
        qkv, kc, vc = RR.random_extend_ragged(HEADS, TMAX, positions, Tn, torch.float32, seed=9)
        out, k2, v2 = RR.extend_ragged_attention_ref(qkv, kc, vc, positions, True)
        for b in range(3):
            rows = out[b * Tn:(b + 1) * Tn]
            if bad[b]:
                assert bool(torch.isnan(rows).all())
                assert torch.equal(DR.bits(k2[b]), DR.bits(kc[b])) and torch.equal(DR.bits(v2[b]), DR.bits(vc[b]))
            else:
                assert bool(torch.isfinite(rows).all()) and not torch.equal(DR.bits(k2[b]), DR.bits(kc[b]))
    assert not RR.guarded(0, TMAX, TMAX) and RR.guarded(1, TMAX, TMAX) and RR.guarded(-1, 1, TMAX)


def test_the_gpu_inputs_tell_one_p_for_the_whole_batch_from_the_right_kernel():
    """A kernel that reads positions[0] (or the largest position) for every sequence must miss the reference by far more than the
    bound, or be NaN (it reads poisoned rows), on every case whose positions differ."""
    for positions, Tn in (((0, 63, 200), 1), ((1, 64, 65), 2), ((63, 64, 200), 64)):
        qkv, kc, vc = RR.random_extend_ragged(HEADS, TMAX, positions, Tn, torch.float32, seed=20000 + 300 * positions[1] + Tn)
        ref, _, _ = RR.extend_ragged_attention_ref(qkv, kc, vc, positions, True)
        for wrong in (positions[0], max(positions)):
            if wrong + Tn > TMAX:
                continue
            got, _, _ = ER.extend_attention_ref(qkv, kc, vc, wrong, True)
            for b, P in enumerate(positions):
                if P == wrong:
                    continue
                rows = slice(b * Tn, (b + 1) * Tn)
                e = DR.rel_err64(got[rows].float(), ref[rows])
                assert not e < 100 * BOUND, (positions, Tn, wrong, b, e)      # (NaN counts as a miss)

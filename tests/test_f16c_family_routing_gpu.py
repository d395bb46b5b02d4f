"""Which KX_PREC_F16C launches each GEMM family of tuning key 16 reaches (kx_gemm_args.f16c_corr; DESIGN §5 "one correction
instead of two, family by family").  Two bits per family — 0 decoder qkv, 1 out_proj, 2 fc1, 3 fc2, 4 output projection,
5 every Perceiver GEMM; the vision tower's launches belong to none.  Family f alone is switched to KX_CORR_NONE (plain fp16
on the same rows) and the stages are compared bit for bit with the shipped assignment: the kernels are deterministic, so
"that family's launches were reached" is "the result changed" and "no other launch was" is "it did not"."""
import pytest
import torch

from helpers import tiny_config  # noqa: F401  (sys.path set up by conftest)
from kosmosx import _hip, ops
from kosmosx.model import Kosmos

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = ["qkv", "out_proj", "fc1", "fc2", "logits", "perceiver"]
KX_TUNE_F16C_CORR, KX_CORR_NONE = 16, 3


def _stages(m, tok, img, vit_default=None):
    """(vision tower alone, Perceiver + image_proj alone on a FIXED input, the full model's logits)"""
    vit = m.clip_model.run(img, m.precision, m._ws).clone()
    per, _ = m.perceive.run(vit if vit_default is None else vit_default, m.precision, m._ws, m.image_proj.weight)
    per = per.clone()
    logits = m(tok, img).clone()
    torch.cuda.synchronize()
    return vit, per, logits


def test_key16_reaches_exactly_the_launches_of_its_family():
    m = Kosmos._from_config(tiny_config(), seed=0, perturb=0.1).eval().to(DEV)
    m.precision = "f16c"            # explicit: every GEMM width of the tiny config is a multiple of 128, no stage falls back
    m.use_hip_graphs = False        # a replayed graph would keep the assignment it was captured with
    g = torch.Generator().manual_seed(16)
    tok = torch.randint(0, m.cfg.vocab, (2, 6), generator=g).to(DEV)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).to(DEV)
    lib = _hip.load()
    vit0, per0, logits0 = _stages(m, tok, img)
    assert torch.isfinite(logits0).all()
    results = []
    for f, name in enumerate(FAMILIES):
        assert lib.kx_set_tuning(KX_TUNE_F16C_CORR, KX_CORR_NONE << (2 * f)) == 0
        try:
            vit, per, logits = _stages(m, tok, img, vit0)
        finally:
            lib.kx_set_tuning(KX_TUNE_F16C_CORR, 0)
        assert torch.equal(vit, vit0), f"family {name}: the vision tower has no family and must not change"       # (a)
        assert torch.equal(per, per0) == (f != 5), f"family {name}: the Perceiver changes for family 5 alone"     # (b)
        assert not torch.equal(logits, logits0), f"family {name}: none of its launches was reached"               # (c)
        assert torch.isfinite(logits).all()
        results.append(logits)
    for i in range(len(results)):                                                                                  # (d)
        for j in range(i + 1, len(results)):
            assert not torch.equal(results[i], results[j]), f"families {FAMILIES[i]} and {FAMILIES[j]} reach the same launches"
    assert torch.equal(_stages(m, tok, img)[2], logits0)           # the key is back at the shipped assignment
    assert ops.pair_split_errors() == 0

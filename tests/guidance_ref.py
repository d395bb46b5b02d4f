"""NumPy restatement of kx_guidance_logits' contract (include/kosmosx_hip.h, "Classifier-free guidance"), written from the contract.

guided_row_f32 is the combine alone, over log-probs the caller brings (the device's own, from kx_token_logprob, in the bit-exact
tests): three separate fp32 operations and the non-finite rule.  guided_row_f64 is the whole rule in float64 from the raw logits."""
import numpy as np


def guided_row_f32(lc, lu, s):
    """out_i = lu_i + s * (lc_i - lu_i): a subtract, a multiply and an add, each rounded to fp32; not finite -> -inf."""
    lc, lu, s = np.asarray(lc, dtype=np.float32), np.asarray(lu, dtype=np.float32), np.float32(s)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (lc - lu).astype(np.float32)
        t = (s * d).astype(np.float32)
        g = (lu + t).astype(np.float32)
    return np.where(np.isfinite(g), g, np.float32(-np.inf)).astype(np.float32)


def log_softmax_f64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = x - x.max(axis=-1, keepdims=True)
        return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def guided_row_f64(c, u, s):
    """float64 log-softmax of both rows, then lu + s * (lc - lu); not finite -> -inf."""
    lc, lu = log_softmax_f64(c), log_softmax_f64(u)
    with np.errstate(invalid="ignore", over="ignore"):
        g = lu + float(s) * (lc - lu)
    return np.where(np.isfinite(g), g, -np.inf)

"""Per-row sampling options without a GPU: generation.check_row_options and generate()'s refusals (which come before the device
check), the public signatures, and the host-only half of the new ABI — kx_sample_rows_pack, which touches no device, and the
argument checks of kx_sample_logits_rows, which come before any launch."""
import ctypes as C
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from kosmosx import generation as G

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "kosmosx_hip.h").read_text()
KX_ERR_INVALID_ARG = 1                                      # include/kosmosx_hip.h, kx_status
NAN = float("nan")
V, B, N = 102, 3, 8


def check(rows, **kw):
    return G.check_row_options(V, B, row_options=rows, max_new_tokens=N, **kw)


# ---- check_row_options ----

BAD_VALUES = [("temperature", True), ("temperature", -0.5), ("temperature", "1"), ("temperature", NAN), ("temperature", 1e39),
              ("top_p", 0), ("top_p", 0.0), ("top_p", 1e-50), ("top_p", False), ("top_k", 2.5), ("top_k", True), ("top_k", 2 ** 31),
              ("repetition_penalty", 0.0), ("repetition_penalty", NAN), ("repetition_penalty", float("inf")),
              ("min_p", -0.1), ("min_p", 1.5), ("min_p", True), ("typical_p", 0), ("typical_p", 1.5), ("typical_p", True),
              ("epsilon_cutoff", 1), ("epsilon_cutoff", -1e-3), ("eta_cutoff", 1.0), ("eta_cutoff", NAN),
              ("presence_penalty", NAN), ("presence_penalty", 1e39), ("frequency_penalty", NAN), ("frequency_penalty", "x"),
              ("seed", 1.5), ("seed", True), ("do_sample", 1), ("do_sample", None),
              ("max_new_tokens", 0), ("max_new_tokens", N + 1), ("max_new_tokens", True), ("max_new_tokens", 2.0)]


@pytest.mark.parametrize("key,value", BAD_VALUES, ids=[f"{k}-{v!r}" for k, v in BAD_VALUES])
def test_a_value_the_scalar_keyword_would_refuse_is_refused_by_name(key, value):
    for b in range(B):
        rows = [{} for _ in range(B)]
        rows[b] = {"seed": 3, key: value}
        with pytest.raises(ValueError, match=re.escape(f"row_options[{b}]['{key}']")):
            check(rows)


def test_the_shape_of_the_argument_is_checked():
    with pytest.raises(ValueError, match=re.escape("row_options[1]['top_q']")):
        check([{}, {"top_q": 0.5}, {}])                                         # an unknown key
    for rows in ([{}] * (B - 1), [{}] * (B + 1), []):                          # a wrong length
        with pytest.raises(ValueError, match=f"row_options must have {B} entries"):
            check(rows)
    for entry in (None, 0.5, [("seed", 1)], "seed"):                           # a non-dict entry
        with pytest.raises(ValueError, match=re.escape("row_options[2] must be a dict")):
            check([{}, {}, entry])
    for whole in ({"seed": 1}, "abc", 7):
        with pytest.raises(ValueError, match="row_options must be a sequence"):
            check(whole)


def test_beams_lookup_and_greedy_parallel_rows_are_refused():
    rows = [{"temperature": 0.7}, {}, {}]
    with pytest.raises(ValueError, match="row_options.*num_beams = 2"):
        check(rows, num_beams=2)
    with pytest.raises(ValueError, match="row_options.*prompt_lookup_num_tokens = 2"):
        check(rows, prompt_lookup_num_tokens=2)
    for greedy in ({"temperature": 0.0}, {"temperature": 0}, {"do_sample": False}):
        with pytest.raises(ValueError, match=re.escape("row_options[1]") + ".*greedy.*num_return_sequences = 2"):
            check([{}, greedy, {}], num_return_sequences=2, do_sample=True)
    assert check(rows, num_return_sequences=2, do_sample=True) is not None
    assert check([{}, {"temperature": 0.0}, {}], do_sample=True) is not None   # a greedy row is fine in the plain loop


def test_none_and_empty_dicts_resolve_to_nothing():
    assert check(None) is None
    assert check([{} for _ in range(B)]) is None
    assert check(tuple({} for _ in range(B)), do_sample=True, temperature=0.7) is None
    assert G.loop_options(V, B).rows is None
    assert G.loop_options(V, B, row_options=[{}] * B, do_sample=True).rows is None


def test_a_row_takes_the_calls_scalars_for_what_it_does_not_name():
    call = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.9, repetition_penalty=1.2, seed=5, min_p=0.05, typical_p=0.95,
                epsilon_cutoff=1e-3, eta_cutoff=2e-3, presence_penalty=0.25, frequency_penalty=-0.5)
    rows = check([{}, {"temperature": 0, "max_new_tokens": 2}, {"seed": 2 ** 63 + 1, "top_k": 0, "frequency_penalty": 1}], **call)
    assert set(rows[0]) == set(G.ROW_KEYS) and len(G.ROW_KEYS) == 13
    assert rows[0] == dict(call, max_new_tokens=0)                               # no budget: the call's own max_new_tokens
    assert rows[1] == dict(call, temperature=0.0, max_new_tokens=2)
    assert rows[2] == dict(call, seed=2 ** 63 + 1, top_k=0, frequency_penalty=1.0, max_new_tokens=0)
    assert check([{"max_new_tokens": N}, {}, {}])[0]["max_new_tokens"] == N     # the call's own value is a budget like any other
    opts = G.loop_options(V, B, row_options=[{}, {"top_p": 0.5}, {}], max_new_tokens=N, **call)
    assert opts.rows[1]["top_p"] == 0.5 and opts.rows[0]["top_p"] == 0.9 and opts.top_p == 0.9
    assert G.loop_options(V, B, row_options=[{"max_new_tokens": 50}, {}, {}]).rows[0]["max_new_tokens"] == 50   # no bound given, none checked


def _sessions(batch=B):
    from kosmosx.model import KosmosLanguage
    lm = KosmosLanguage(vocab_size=V, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    return [G.Session(lm, {"batch": batch}, 20)]


def _models(batch=B):
    from helpers import tiny_config
    from kosmosx.model import Kosmos, KosmosLanguage
    lm = KosmosLanguage(vocab_size=V, dim=128, depth=1, ffn_dim=128, decoder_heads=2, _seed=0, _max_positions=32).eval()
    m = Kosmos._from_config(tiny_config(), seed=0).eval()
    tok = torch.zeros(batch, 4, dtype=torch.long)
    img = torch.zeros(batch, 3, m.cfg.vit.image, m.cfg.vit.image)
    session = [G.Session(model, {"batch": batch}, 20) for model in (lm, m)]
    return [(lambda **kw: lm.generate(tok, 4, **kw)), (lambda **kw: m.generate(tok, img, 4, **kw)),
            (lambda **kw: session[0].generate(tok, 4, **kw)), (lambda **kw: session[1].generate(tok, 4, **kw))]


def test_generate_refuses_before_the_device_check_and_good_values_reach_it():
    """CPU tensors, for Kosmos, KosmosLanguage and Session."""
    gens = _models()
    for gen in gens:
        with pytest.raises(ValueError, match=re.escape("row_options[0]['top_p']")):
            gen(row_options=[{"top_p": 0}, {}, {}])
        with pytest.raises(ValueError, match=re.escape("row_options[2]['max_new_tokens']")):
            gen(row_options=[{}, {}, {"max_new_tokens": 5}])                    # above the call's 4
        with pytest.raises(ValueError, match="row_options must have 3 entries"):
            gen(row_options=[{}])
        with pytest.raises(ValueError, match="typical_p"):                      # the scalar checks come first, unchanged
            gen(typical_p=0, row_options=[{"top_p": 0}, {}, {}])
        for good in ([{"temperature": 0.5, "do_sample": True}, {"max_new_tokens": 2}, {}], [{}, {}, {}], None):
            with pytest.raises(RuntimeError, match="CUDA|HIP|fallback"):
                gen(row_options=good)
    for gen in gens[:2]:
        with pytest.raises(ValueError, match="row_options.*num_beams"):
            gen(num_beams=2, row_options=[{"seed": 1}, {}, {}])
        with pytest.raises(ValueError, match="row_options.*prompt_lookup_num_tokens"):
            gen(prompt_lookup_num_tokens=2, row_options=[{"seed": 1}, {}, {}])
        with pytest.raises(ValueError, match="row_options.*greedy"):
            gen(num_return_sequences=2, do_sample=True, row_options=[{"temperature": 0}, {}, {}])


def test_a_bad_max_new_tokens_of_the_call_is_refused_in_its_own_words():
    """The budgets take no bound from a call's value that is no positive integer: that value's own check speaks."""
    rows = [{"max_new_tokens": 1}, {}, {}]
    for bad in (0, -2, True, 2.5, None):
        assert G.check_row_options(V, B, row_options=rows, max_new_tokens=bad)[0]["max_new_tokens"] == 1
    tok = torch.zeros(B, 4, dtype=torch.long)
    for model in _sessions():
        for bad in (0, True):
            with pytest.raises(ValueError, match="max_new_tokens must be a positive integer"):
                model.generate(tok, bad, row_options=rows)


def test_the_signatures_carry_the_keyword():
    from kosmosx import ops
    from kosmosx.model import Kosmos, KosmosLanguage
    for fn in (Kosmos.generate, KosmosLanguage.generate, G.Session.generate, G.loop_options, G.check_row_options):
        p = inspect.signature(fn).parameters["row_options"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
    assert inspect.signature(ops.sample_logits).parameters["rows"].default is None
    for name in ("frequency_rows", "presence_rows"):
        assert inspect.signature(ops.shape_logits).parameters[name].default is None
    assert [f.name for f in __import__("dataclasses").fields(G.LoopOptions)][-1] == "rows"


# ---- the C ABI ----

@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kx_build", ROOT / "kosmos-x_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from kosmosx import _hip
    return _hip.load()


def test_the_header_declares_the_abi_and_the_mirrors_list_the_fields_in_order(lib):
    from kosmosx import _hip
    for decl in ("int kx_sample_rows_pack(const kx_sample_row* in, int64_t B, int64_t V, kx_sample_row* out, uint32_t* flags_out);",
                 "int kx_sample_logits_rows(const kx_sample_args* args, int32_t* positions, int64_t advance, const kx_sample_rows_args* rows, "
                 "void* stream);",
                 "int kx_shape_logits_rows(const kx_shape_args* args, const float* frequency_rows, const float* presence_rows, void* stream);"):
        assert decl in HEADER, decl
        name = decl.split("(")[0].split()[-1]
        assert hasattr(lib, name) and name in _hip.SYMBOLS
    assert lib.kx_version() == 7 and "#define KX_ABI_VERSION 7" in HEADER and "KX_STRUCT_COUNT = 13" in HEADER   # appended within ABI 7
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for struct, mirror in (("kx_sample_row", _hip.SampleRow), ("kx_sample_rows_args", _hip.SampleRowsArgs)):
        m = re.search(r"typedef struct \{([^{}]*)\}\s*" + struct + r"\s*;", body, flags=re.S)
        assert m, struct
        names = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            names += [re.findall(r"([A-Za-z_0-9]+)\s*$", part.replace("*", " ").strip())[0] for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_hip.SampleRow) == 56 and C.alignment(_hip.SampleRow) == 8 and _hip.SampleRow.seed.offset == 48
    assert _hip.SampleRowsArgs().struct_bytes == C.sizeof(_hip.SampleRowsArgs) == 16
    r = _hip.SampleRow()
    assert (r.do_sample, r.temperature, r.top_k, r.top_p, r.repetition_penalty, r.min_p, r.typical_p, r.epsilon_cutoff, r.eta_cutoff,
            r.max_new, r.seed) == (0, 1.0, 0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, 0)


def _pack(lib, records, vocab=V, out=None):
    from kosmosx import _hip
    arr = (_hip.SampleRow * len(records))(*records)
    flags = C.c_uint32(0xdead)
    rc = lib.kx_sample_rows_pack(arr, len(records), vocab, arr if out is None else out, C.byref(flags))
    return rc, flags.value, arr


def test_the_pack_function_needs_no_device_fills_log_min_p_and_sets_the_flags(lib):
    from kosmosx import _hip
    R = _hip.SampleRow
    ms = (1.0, 0.5, 0.25, 0.05, 0.3, 1e-3, 1e-30, 0.9999999)
    rc, flags, arr = _pack(lib, [R(min_p=m, do_sample=1, seed=2 ** 64 - 1 - i) for i, m in enumerate(ms)] + [R()])
    assert rc == 0 and flags == 0
    for rec, m in zip(arr, ms):
        want = np.float32(math.log(float(np.float32(m))))
        assert np.float32(rec.log_min_p).tobytes() == want.tobytes(), m         # the bits of kx_sample_logits_min_p's own expression
        assert rec.min_p == np.float32(m) and rec.do_sample == 1 and rec.reserved == 0
    assert arr[0].log_min_p == 0.0 and arr[0].seed == 2 ** 64 - 1 and arr[len(ms)].log_min_p == 0.0
    assert _pack(lib, [R(), R(repetition_penalty=1.25), R()])[:2] == (0, _hip.SAMPLE_ROWS_PENALTY)
    assert _pack(lib, [R(), R(max_new=3)])[:2] == (0, _hip.SAMPLE_ROWS_BUDGET)
    assert _pack(lib, [R(max_new=1, repetition_penalty=0.5)])[:2] == (0, _hip.SAMPLE_ROWS_PENALTY | _hip.SAMPLE_ROWS_BUDGET)
    dirty = R(min_p=0.5, max_new=2)
    dirty.log_min_p, dirty.reserved = 7.0, 9                                    # what the caller left there does not matter
    out = (R * 1)()
    rc, flags, src = _pack(lib, [dirty], out=out)                               # in != out: the input stays as it was
    assert rc == 0 and src[0].log_min_p == 7.0 and out[0].reserved == 0 and out[0].max_new == 2
    assert np.float32(out[0].log_min_p) == np.float32(math.log(0.5))


BAD_RECORDS = [("temperature", -1.0), ("temperature", NAN), ("top_p", 0.0), ("top_p", -0.5), ("top_p", NAN), ("repetition_penalty", 0.0),
               ("repetition_penalty", NAN), ("min_p", -0.25), ("min_p", 1.5), ("min_p", NAN), ("typical_p", 0.0), ("typical_p", 1.5),
               ("typical_p", NAN), ("epsilon_cutoff", -1e-3), ("epsilon_cutoff", 1.0), ("epsilon_cutoff", NAN), ("eta_cutoff", 1.0),
               ("eta_cutoff", 2.0), ("eta_cutoff", NAN), ("max_new", -1)]


def test_the_pack_function_refuses_a_bad_record_naming_the_row_and_the_field(lib):
    from kosmosx import _hip
    R = _hip.SampleRow
    for name, v in BAD_RECORDS:
        for b in (0, 2):
            recs = [R(), R(), R()]
            recs[b] = R(**{name: v})
            rc, flags, arr = _pack(lib, recs)
            msg = _hip.last_error()
            assert rc == KX_ERR_INVALID_ARG and f"row {b}: {name}" in msg and "kx_sample_rows_pack" in msg, (name, v, b, rc, msg)
            assert flags == 0xdead                                              # nothing is written for a refused table
    ok = (R * 1)()
    flags = C.c_uint32(0)
    for args, word in (((None, 1, V, ok, C.byref(flags)), "null in"), ((ok, 1, V, None, C.byref(flags)), "null out"),
                       ((ok, 1, V, ok, None), "null flags_out"), ((ok, 0, V, ok, C.byref(flags)), "B=0"), ((ok, 1, 0, ok, C.byref(flags)), "V=0")):
        assert lib.kx_sample_rows_pack(*args) == KX_ERR_INVALID_ARG and word in _hip.last_error(), word


def test_the_rows_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """The table pointer is never followed and no device is needed: every refusal comes before the launch."""
    from kosmosx import _hip
    a = _hip.SampleArgs()
    call = lib.kx_sample_logits_rows
    assert call(C.byref(a), None, 0, None, None) == KX_ERR_INVALID_ARG and "null rows" in _hip.last_error()
    stale = _hip.SampleRowsArgs()
    stale.struct_bytes -= 8
    assert call(C.byref(a), None, 0, C.byref(stale), None) == KX_ERR_INVALID_ARG           # a null table: nothing could be read
    assert "stale binding" in _hip.last_error() and "kx_sample_rows_args" in _hip.last_error()
    r = _hip.SampleRowsArgs()
    assert call(C.byref(a), None, 0, C.byref(r), None) == KX_ERR_INVALID_ARG and "null table" in _hip.last_error()
    r = _hip.SampleRowsArgs(table=4096, flags=4)
    assert call(C.byref(a), None, 0, C.byref(r), None) == KX_ERR_INVALID_ARG and "flags" in _hip.last_error()
    r = _hip.SampleRowsArgs(table=4096)
    assert call(C.byref(a), 4096, -1, C.byref(r), None) == KX_ERR_INVALID_ARG and "advance" in _hip.last_error()
    assert call(None, None, 0, C.byref(r), None) == KX_ERR_INVALID_ARG and "null args" in _hip.last_error()
    assert call(C.byref(a), None, 0, C.byref(r), None) == KX_ERR_INVALID_ARG and "null logits" in _hip.last_error()
    # the scalar sampling fields of args are ignored: values kx_sample_logits refuses get as far as the next check
    a.logits, a.next_token, a.B, a.V, a.ld = 4096, 4096, 2, 10, 10
    a.temperature, a.top_p, a.repetition_penalty = -1.0, 0.0, 0.0
    r = _hip.SampleRowsArgs(table=4096, flags=_hip.SAMPLE_ROWS_BUDGET)
    assert call(C.byref(a), None, 0, C.byref(r), None) == KX_ERR_INVALID_ARG and "null finished" in _hip.last_error()
    assert lib.kx_sample_logits(C.byref(a), None) == KX_ERR_INVALID_ARG and "temperature" in _hip.last_error()
    s = _hip.ShapeArgs()
    s.logits, s.B, s.V, s.ld, s.bias_off = 4096, 2, 10, 10, 4096
    assert lib.kx_shape_logits_rows(C.byref(s), 4096, None, None) == KX_ERR_INVALID_ARG and "counts" in _hip.last_error()
    assert lib.kx_shape_logits_rows(C.byref(s), None, 4096, None) == KX_ERR_INVALID_ARG and "counts" in _hip.last_error()

"""hac_index_set_option / hac_encoder_set_option: every option of both handles with its documented values and with values it must
refuse.  The two option tables of the library (csrc/hac_common.h: Option; `Opt::choice(..)`, `Opt::integer(..)` and
`Opt::custom_form(..)` rows in flat_ip.hip and encoder.hip) are mirrored by the two tables below, and a CPU test compares the names,
so an option added later without a row here fails.

The handles that take the values hold no rows and no weights: setting an option launches nothing.  The refused values of the index
go to a second, filled index (128 rows, d = 64, split = "0"), which is searched after every refusal: a refused value must not
half-apply.  Per option: (accepted values, refused values); the accepted lists end at the default.  The refused values include
the empty string, a value of a neighbouring option and, for integers, the first value beyond each end of the range.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "haconvdr_amd", "csrc")

_STREAMS = (("auto", "1", "17", "4096", "auto"), ("", "0", "4097", "-1", "65535", "1.5"))     # the four *_p options
_TILES = (("0", "1", "65535", "0"), ("", "65536", "-1", "auto", "7 "))                          # the four debug_*_tiles options
INDEX_OPTIONS = {
    "split": (("0", "1", "auto"), ("", "2", "host", "01")),
    "split_terms": (("3", "1"), ("", "2", "auto")),
    "force_scan16": (("1", "0"), ("", "auto", "2")),
    "scanq_nt": (("1", "2", "3", "4", "0"), ("", "5", "8", "-1")),
    "scanq_waves": (("4", "8"), ("", "0", "16")),
    "scan_no_p8": (("1", "0"), ("", "auto", "true")),
    "split_decide": (("host", "device", "auto"), ("", "0", "gpu")),
    "scan_pass_cuts": (("1,2", "100,310", "899,900", "auto"), ("", "901,902", "5,5", "0,4", "7", "4,3", "lazy")),
    "scan_passes": (("1", "2", "3", "4", "5", "auto"), ("", "0", "6", "1,2")),
    "scan_halfq": (("0", "1"), ("", "auto", "2")),
    "fp16_image": (("eager", "lazy"), ("", "1", "auto")),
    "rescore_rows": (("0", "1", "auto"), ("", "2", "eager")),
    "debug_oom": (("3", "1000", "0"), ("", "1001", "-1", "auto", "3x")),
    "debug_max_pass": (("1", "1000000", "0"), ("", "-1", "1000001", "auto")),
    "masked_p": _STREAMS,
    "grouped_p": _STREAMS,
    "after_p": _STREAMS,
    "at_rank_p": _STREAMS,
    "debug_masked_tiles": _TILES,
    "debug_grouped_tiles": _TILES,
    "debug_after_tiles": _TILES,
    "debug_at_rank_tiles": _TILES,
    "seed_groups_max": (("1", "768", "5000", str(2 ** 40), "0"), ("", "-1", "auto", "12x")),
}
ENCODER_OPTIONS = {
    "gemm": (("classic", "8phase", "auto"), ("", "gemm8", "split")),
    "precision": (("split", "bf16"), ("", "fp32", "classic")),
    "model": (("bert", "roberta"), ("", "ance", "mean")),
    "pooling": (("mean", "first"), ("", "cls", "bert")),
    "attn": (("twopass", "stream"), ("", "auto", "all")),
    "attn_pipe": (("off", "all", "auto"), ("", "on", "twopass")),
    "attn_qsplit": (("off", "auto"), ("", "on", "all")),
    "g8_stagger": (("off", "auto"), ("", "on", "6")),
    "attn_qs_pin": (("1", "2", "4", "8", "16", "0"), ("", "3", "32", "auto")),
    "ksplit_pin": (("2/4", "16/16", "0/16", "0/0"), ("", "17/1", "1/17", "-1/2", "4", "off")),
    "ksplit": (("off", "auto"), ("", "on", "2/4")),
    "graph": (("off", "auto"), ("", "on", "replay")),
    "max_tokens": (("4096", "8192", "524288"), ("", "4095", "auto", "-1", "4096x")),
}


def test_every_option_of_the_library_has_a_row_here():
    row = re.compile(r'\bOpt::(?:choice|integer|custom_form)\("([a-z0-9_]+)"')
    for src, mine in (("flat_ip.hip", INDEX_OPTIONS), ("encoder.hip", ENCODER_OPTIONS)):
        names = row.findall(open(os.path.join(CSRC, src)).read())
        assert len(names) == len(set(names)), f"{src}: an option has two rows"
        assert set(names) == set(mine), (src, set(names) ^ set(mine))
    for name, (accepted, refused) in list(INDEX_OPTIONS.items()) + list(ENCODER_OPTIONS.items()):
        assert len(accepted) >= 2 and len(refused) >= 2 and "" in refused and not set(accepted) & set(refused), name


@pytest.fixture(scope="module")
def empty_index():
    from haconvdr_amd.index import FlatIPIndex
    return FlatIPIndex(d=32)


@pytest.fixture(scope="module")
def encoder():
    from haconvdr_amd.encoder import ANCEEncoder
    return ANCEEncoder()


@pytest.fixture(scope="module")
def filled():
    """(index of 128 rows at split = "0", its queries, what the search returned before any refusal)"""
    from haconvdr_amd.index import FlatIPIndex
    rng = np.random.default_rng(20261021)
    idx = FlatIPIndex(d=64)
    idx.add(rng.standard_normal((128, 64), dtype=np.float32))
    idx.set_option("split", "0")
    q = rng.standard_normal((3, 64), dtype=np.float32)
    return idx, q, idx.search(q, 4)


def _refused(handle, name, value):
    from haconvdr_amd import _lib
    with pytest.raises(_lib.HacError) as e:
        handle.set_option(name, value)
    assert e.value.code == _lib.HAC_ERR_INVALID, (name, value, e.value.code)
    assert f"{name} = '{value}'" in str(e.value), (name, value, str(e.value))   # (a stale message names another option or value)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INDEX_OPTIONS))
def test_index_option(name, empty_index, filled):
    accepted, refused = INDEX_OPTIONS[name]
    for v in accepted:
        empty_index.set_option(name, v)
    idx, q, (D0, I0) = filled
    for v in refused:
        assert "index option" in _refused(empty_index, name, v)
        _refused(idx, name, v)
        D, I = idx.search(q, 4)
        assert np.array_equal(I, I0) and np.array_equal(D, D0), (name, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ENCODER_OPTIONS))
def test_encoder_option(name, encoder):
    accepted, refused = ENCODER_OPTIONS[name]
    for v in accepted:
        encoder.set_option(name, v)
    for v in refused:
        assert "encoder option" in _refused(encoder, name, v)


@pytest.mark.gpu
def test_unknown_names(empty_index, encoder, filled):
    from haconvdr_amd import _lib
    idx, q, (D0, I0) = filled
    for handle in (empty_index, encoder, idx):
        for name in ("", "no_such_option", "Split", "split "):
            with pytest.raises(_lib.HacError) as e:
                handle.set_option(name, "0")
            assert e.value.code == _lib.HAC_ERR_INVALID and "unknown" in str(e.value) and f"'{name}'" in str(e.value), (name, str(e.value))
    D, I = idx.search(q, 4)
    assert np.array_equal(I, I0) and np.array_equal(D, D0)


@pytest.mark.gpu
def test_model_is_refused_after_a_weight():
    from haconvdr_amd import _lib
    from haconvdr_amd.encoder import ANCEEncoder
    enc = ANCEEncoder()
    enc.set_option("model", "bert")
    enc.set_option("model", "roberta")
    w = np.zeros(4, np.float32)
    _lib.check(_lib.lib().hac_encoder_set_weight(enc._h, b"norm.bias", w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), w.size))
    for v in ("bert", "roberta"):
        assert "hac_encoder_set_weight" in _refused(enc, "model", v)
    enc.set_option("pooling", "mean")   # (the other options stay open)

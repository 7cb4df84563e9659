"""CPU-side checks of ``keep_fp16`` (LlamaHIP(weight_format="mxfp4", keep_fp16=False): only the 4-bit images stay resident): the
refusals are raised by the pure check next to ``check_weight_format`` -- before anything is allocated -- and ``PC_W4_KEEP_FP16``
parses to the documented values."""
import inspect

import pytest


def _m():
    from promptcache_amd.model import llama_hip
    return llama_hip


def test_keep_fp16_false_needs_mxfp4():
    with pytest.raises(ValueError, match="weight_format='mxfp4'"):
        _m().check_keep_fp16(False, "fp16", env={})


def test_keep_fp16_false_excludes_w4_stream_0():
    with pytest.raises(ValueError, match="PC_W4_STREAM=0"):
        _m().check_keep_fp16(False, "mxfp4", env={"PC_W4_STREAM": "0"})
    with pytest.raises(ValueError, match="PC_W4_STREAM=0"):
        _m().check_keep_fp16(None, "mxfp4", env={"PC_W4_STREAM": "0", "PC_W4_KEEP_FP16": "0"})


def test_keep_fp16_false_excludes_dense_lo8():
    with pytest.raises(ValueError, match="PC_DENSE_LO8=1"):
        _m().check_keep_fp16(False, "mxfp4", env={"PC_DENSE_LO8": "1"})


def test_accepted_combinations():
    m = _m()
    assert m.check_keep_fp16(False, "mxfp4", env={}) is False
    assert m.check_keep_fp16(False, "mxfp4", env={"PC_W4_STREAM": "1", "PC_DENSE_LO8": "0"}) is False
    assert m.check_keep_fp16(True, "fp16", env={"PC_W4_STREAM": "0", "PC_DENSE_LO8": "1"}) is True
    assert m.check_keep_fp16(True, "mxfp4", env={"PC_W4_STREAM": "0", "PC_W4_KEEP_FP16": "0"}) is True      # the argument wins
    assert m.check_keep_fp16(None, "mxfp4", env={}) is True                                                 # default: today's model
    assert m.check_keep_fp16(None, "mxfp4", env={"PC_W4_KEEP_FP16": "0"}) is False
    assert m.check_keep_fp16(None, "fp16", env={"PC_W4_KEEP_FP16": "0"}) is True      # the variable speaks about MXFP4 models only


@pytest.mark.parametrize("value,want", [(None, True), ("", True), ("1", True), ("0", False)])
def test_pc_w4_keep_fp16_parsing(value, want):
    assert _m().parse_keep_fp16(value) is want


@pytest.mark.parametrize("value", ["no", "false", "2", " 0"])
def test_pc_w4_keep_fp16_rejects_anything_else(value):
    with pytest.raises(ValueError, match="PC_W4_KEEP_FP16"):
        _m().parse_keep_fp16(value)


def test_environment_form_reads_os_environ(monkeypatch):
    monkeypatch.setenv("PC_W4_KEEP_FP16", "0")
    monkeypatch.delenv("PC_W4_STREAM", raising=False)
    monkeypatch.delenv("PC_DENSE_LO8", raising=False)
    assert _m().check_keep_fp16(None, "mxfp4") is False
    monkeypatch.setenv("PC_W4_STREAM", "0")
    with pytest.raises(ValueError, match="PC_W4_STREAM=0"):
        _m().check_keep_fp16(None, "mxfp4")


def test_constructor_takes_keep_fp16_and_refuses_before_allocating():
    """The constructor has the argument and raises from the pure check: an fp16 model with keep_fp16=False never touches its
    weights (an empty dict) or a device."""
    m = _m()
    assert "keep_fp16" in inspect.signature(m.LlamaHIP.__init__).parameters
    from promptcache_amd.model.config import SHAPES
    with pytest.raises(ValueError, match="keep_fp16=False"):
        m.LlamaHIP(SHAPES["mid64"], {}, device="cpu", weight_format="fp16", keep_fp16=False)

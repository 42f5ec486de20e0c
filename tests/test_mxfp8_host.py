"""CPU: the opt-in MX-fp8 linear layers' host side -- argument validation of wf_mx_quant_e4m3 / wf_gemm_mxfp8 (every rejected call returns
WF_EINVAL before any device work; there is no fallback), the precision switches of both DiTs and of the inference entry point."""
import pytest

from worldforge_amd import _ffi

EINVAL = -1
A16 = 1 << 20  # a 16-byte aligned fake address: never dereferenced, every call below is rejected first


def _gemm(**kw):
    a = dict(Xq=A16, Xs=A16, Wq=A16, Ws=A16, bias=None, out=A16, gate=None, M=256, N=256, K=256, ldx=256, ldw=256, ldo=256, epi=0)
    a.update(kw)
    return _ffi.lib().wf_gemm_mxfp8(a["Xq"], a["Xs"], a["Wq"], a["Ws"], a["bias"], a["out"], a["gate"], a["M"], a["N"], a["K"], a["ldx"],
                                    a["ldw"], a["ldo"], a["epi"], None)


@pytest.mark.parametrize("bad", [
    dict(K=192, ldx=192, ldw=192),      # K % 128 != 0
    dict(K=64, ldx=64, ldw=64),
    dict(epi=4), dict(epi=-1), dict(epi=7),  # unknown epilogue (EPI_F32_ACC is not built for MX-fp8)
    dict(Xq=A16 + 8), dict(Wq=A16 + 4), dict(out=A16 + 8), dict(bias=A16 + 4), dict(gate=A16 + 12),  # misaligned operands
    dict(Xs=A16 + 2), dict(Ws=A16 + 1),    # misaligned scales
    dict(ldx=264), dict(ldw=200), dict(ldx=128),  # ld not a multiple of 16, or < K
    dict(N=258, ldo=258), dict(ldo=128),   # N % 4, ldo < N
    dict(M=0), dict(Xq=None), dict(Ws=None),
])
def test_gemm_mxfp8_rejects(bad):
    assert _gemm(**bad) == EINVAL
    assert _ffi.lib().wf_last_error()


@pytest.mark.parametrize("M,K,ldx,X,Q", [(4, 48, 48, A16, A16), (4, 64, 60, A16, A16), (4, 64, 64, A16 + 8, A16), (4, 64, 64, A16, A16 + 4),
                                         (0, 64, 64, A16, A16)])
def test_mx_quant_rejects(M, K, ldx, X, Q):
    assert _ffi.lib().wf_mx_quant_e4m3(X, Q, A16, M, K, ldx, None) == EINVAL


def test_precision_switches():
    from worldforge_amd.dit import DiTConfig, WanTransformer3DModel
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    cfg = DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    assert WanTransformer3DModel(cfg, "cpu").linear_precision == "bf16"
    assert WanTransformer3DModel(cfg, "cpu", linear_precision="mxfp8").linear_precision == "mxfp8"
    lcfg = LongCatConfig(hidden_size=256, depth=1, num_heads=2, caption_channels=64, adaln_tembed_dim=64)
    assert LongCatVideoTransformer3DModel(lcfg, "cpu").linear_precision == "bf16"
    assert LongCatVideoTransformer3DModel(lcfg, "cpu", linear_precision="mxfp8").linear_precision == "mxfp8"
    with pytest.raises(ValueError):
        WanTransformer3DModel(cfg, "cpu", linear_precision="fp8")
    with pytest.raises(ValueError):
        LongCatVideoTransformer3DModel(lcfg, "cpu", linear_precision="int8")


def test_infer_dit_precision_flag(monkeypatch):
    from worldforge_amd import infer
    seen = {}

    def fake_run(*a, **kw):
        seen.update(kw)
        return [], None

    monkeypatch.setattr(infer, "run", fake_run)
    base = ["--models-dir", "m", "--video-ref", "v"]
    infer.main(base)
    assert seen["dit_precision"] == "bf16"
    infer.main(base + ["--dit-precision", "mxfp8"])
    assert seen["dit_precision"] == "mxfp8"
    with pytest.raises(SystemExit):
        infer.main(base + ["--dit-precision", "fp4"])

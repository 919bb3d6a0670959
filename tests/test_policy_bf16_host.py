"""CPU: the bf16 front end (csrc/mrca_policy_bf16.hip) as compiled for gfx950 -- bf16 MFMAs and no fp32 ones, no scratch,
registers for the two waves per SIMD its design counts on -- its C ABI's argument checks (no device touched), and the
test reference's rounding helper against torch's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bf16_ref as R
import util as U

CSRC = os.path.join(U.ROOT, "rl-collision-avoidance_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MRCA_ERR_INVALID, MRCA_ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "mrca_policy_bf16.s"
    build = open(os.path.join(CSRC, "build.sh")).read()
    flags = " ".join(re.findall(r"^\s+(-f[\w=-]+(?:\s+-f[\w=-]+)*)", build, re.M)).split()
    assert "-ffp-contract=off" in flags and "mrca_policy_bf16" in build
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "-S", "--cuda-device-only",
                    os.path.join(CSRC, "mrca_policy_bf16.hip"), "-o", str(out)], check=True, capture_output=True)
    return open(out).read()


def _kernels(asm):
    """-> {kernel name: metadata text} of the bf16 front end's instantiations"""
    meta = asm[asm.index("amdhsa.kernels:"):]
    parts = re.split(r"\n  - ", meta)
    return {re.search(r"\.name:\s+(\S+)", p).group(1): p for p in parts if "lidar_features_bf16_kernel" in p and ".name:" in p}


def test_bf16_mfmas_only(isa):
    assert isa.count("v_mfma_f32_32x32x16_bf16") >= 2 * (16 + 24)        # two instantiations (RAW or not)
    assert "v_mfma_f32_32x32x2_f32" not in isa
    assert "v_cvt_pk_bf16_f32" in isa                                       # the rounding points are plain casts


def test_no_scratch_and_two_waves_per_simd(isa):
    ks = _kernels(isa)
    assert len(ks) == 2
    for name, m in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", m).group(1)) == 0, name
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", m).group(1))
        agpr = int(re.search(r"\.agpr_count:\s+(\d+)", m).group(1))
        assert vgpr + agpr <= 256, (name, vgpr, agpr)                    # 512 registers per SIMD lane: 2 waves


def test_abi_checks_arguments_before_touching_a_device(built_lib):
    f = built_lib.mrca_lidar_features_bf16
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    p = 4096                                         # never dereferenced: the checks come first
    assert f(p, None, 0, 8, 2, 512, p, p, p, p, p, None) == MRCA_ERR_UNSUPPORTED
    assert f(p, None, 0, 8, 3, 256, p, p, p, p, p, None) == MRCA_ERR_UNSUPPORTED
    assert "frames" in built_lib.mrca_last_error().decode()
    assert f(None, None, 0, 8, 3, 512, p, p, p, p, p, None) == MRCA_ERR_INVALID
    assert f(p, None, 0, 8, 3, 512, p, p, p, p, None, None) == MRCA_ERR_INVALID
    assert f(p, None, 0, 8, 3, 512, p, p, p, p, p + 2, None) == MRCA_ERR_INVALID         # feat not 16-byte aligned


def test_symbol_declared_and_exported(built_lib):
    from mrca import _lib
    hdr = open(os.path.join(U.ROOT, "include", "mrca_env.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in _lib.EXPORTS_WITH_DIGITS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert hasattr(built_lib, name), name
    assert sorted(set(re.findall(r"\b(mrca_\w*\d\w*)\s*\(", hdr))) == sorted(_lib.EXPORTS_WITH_DIGITS)


def test_rne_helper_agrees_with_torch():
    rng = np.random.default_rng(0)
    bits = np.concatenate([
        rng.integers(0, 2 ** 32, 200000, dtype=np.uint64),
        # ties: the low 16 bits exactly 0x8000, with even and odd bf16 mantissas, both signs
        (rng.integers(0, 2 ** 16, 4000, dtype=np.uint64) << 16) | 0x8000,
        # subnormals and the smallest normals
        rng.integers(0, 0x00820000, 4000, dtype=np.uint64), rng.integers(0x80000000, 0x80820000, 4000, dtype=np.uint64),
        # large values: near the top of the range, where rounding overflows to infinity
        rng.integers(0x7F700000, 0x7F800000, 4000, dtype=np.uint64), rng.integers(0xFF700000, 0xFF800000, 4000, dtype=np.uint64),
        np.array([0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0x7F800000, 0xFF800000],
                 dtype=np.uint64),
    ]).astype(np.uint32)
    a = bits.view(np.float32)
    a = a[~np.isnan(a)]
    mine = R.rne_bf16(a)
    ref = torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32))
    assert np.isnan(R.rne_bf16(np.array([np.nan], np.float32))).all()

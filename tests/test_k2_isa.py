"""What the compiler made of the single-end two-isoform kernels (CPU): no scratch, no spilled vector registers, and the
narrow kernel within the registers of three wavefronts per SIMD.

The build keeps the assembly of the headline's unit and of the narrow one (miso_amd/csrc/Makefile, K2M_ISA ->
miso_amd/csrc/.isa/kernels_k2m_m0w8.s, kernels_k2m_m0w4n.s); the figures are the code object's own metadata at its end.
"""
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "miso_amd", "csrc", ".isa")
UNITS = ("kernels_k2m_m0w8", "kernels_k2m_m0w4n")
FIELDS = ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")


def _kernels(path):
    """{mangled kernel name: {field: value}} from the amdhsa.kernels metadata of one assembly file."""
    out, cur = {}, {}
    with open(path) as f:
        for line in f:
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
            if not m:
                continue
            key, val = m.groups()
            if key in FIELDS:
                cur[key] = int(val)
            elif key == "name" and val.startswith("_Z"):   # (the kernel's own name; its arguments' .name entries are plain)
                cur["name"] = val
            if key == "wavefront_size":                    # last field of a kernel's record
                if "name" in cur:
                    out[cur["name"]] = cur
                cur = {}
    return out


def _assembly():
    paths = [os.path.join(ISA, u + ".s") for u in UNITS]
    if not all(os.path.exists(p) for p in paths):
        hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc on this machine and no assembly kept by a build")
        pytest.skip("the build kept no assembly of the two-isoform units (make -C miso_amd/csrc)")
    return paths


def test_single_end_two_isoform_kernels_have_no_scratch_and_the_narrow_one_fits_three_wavefronts():
    seen = {}
    for p in _assembly():
        for name, k in _kernels(p).items():
            if "sampler_k2_multi" in name:
                seen[name] = k
    # sampler_k2_multi<0, 8>, and <0, 4, true> (Itanium mangling: ILi0ELi8ELb0E, ILi0ELi4ELb1E)
    wide = [k for n, k in seen.items() if "ILi0ELi8ELb0E" in n]
    narrow = [k for n, k in seen.items() if "ILi0ELi4ELb1E" in n]
    assert len(wide) == 1 and len(narrow) == 1, sorted(seen)
    for name, k in seen.items():
        assert set(FIELDS) <= set(k), (name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
    assert narrow[0]["vgpr_count"] <= 168, narrow[0]     # three wavefronts per SIMD: 512 / 3, in units of 8
    assert wide[0]["vgpr_count"] <= 256, wide[0]

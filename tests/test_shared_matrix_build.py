"""Build-time properties of the passes over A (kernels_gemv.hip: gemv_n_kernel, gemv_t_kernel, gemv_dual_kernel, each
one template for members that own their A -- groups of one -- and for groups of members that share one A): every
instantiation exists and carries NO VGPR / SGPR spill and no scratch -- a group of members is held in registers, and a
spill would put a scratch round trip into every step of a pass that exists to save memory traffic -- and keeps at least
the waves per SIMD it was written for.  Read from hipcc's own resource-usage remarks; no GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# template arguments as they stand in the mangled name -> least waves per SIMD
#   gemv_n_kernel<NRHS, RPW, SG, SHARED>, gemv_t_kernel<NRHS, SG, SHARED>, gemv_dual_kernel<CW, SG, SHARED>
WAVES_PER_SIMD = {
    "gemv_n_kernel": {(1, 1, 1, 0): 8, (1, 2, 1, 0): 8, (2, 1, 1, 0): 8, (2, 2, 1, 0): 8,
                      (1, 1, 4, 1): 8, (1, 4, 4, 1): 7, (2, 1, 4, 1): 7, (2, 4, 4, 1): 3},
    "gemv_t_kernel": {(1, 1, 0): 8, (2, 1, 0): 8, (1, 8, 1): 6, (2, 8, 1): 3},
    "gemv_dual_kernel": {(1024, 1, 0): 3, (256, 1, 0): 5, (1024, 2, 1): 2, (256, 4, 1): 2},
}


def test_shared_matrix_kernels_have_no_spills():
    src = os.path.join(ROOT, "lp_amd", "csrc", "kernels_gemv.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull],
                         capture_output=True, text=True, cwd=os.path.dirname(src)).stderr
    blocks = re.split(r"remark: Function Name: ", out)
    for name, floors in WAVES_PER_SIMD.items():
        found = {}
        for b in blocks[1:]:
            m = re.match(r"_ZN5lpipm\d+" + name + r"I((?:L[ib]\d+E)+)E", b)
            if m:
                found[tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))] = b
        assert sorted(found) == sorted(floors), (name, [b.splitlines()[0] for b in blocks[1:]])
        for args, b in found.items():
            get = lambda key: int(re.search(key + r": (\d+)", b).group(1))
            assert get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, b
            assert get(r"Occupancy \[waves/SIMD\]") >= floors[args], (name, args, b)


def test_planted_scenarios_have_their_planted_optimum():
    """synth.planted_scenarios: planted_lp's A, and per scenario a strictly complementary primal-dual pair (x*, y*, z*)."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
    from lp_amd import synth
    m, n, K = 24, 60, 5
    A, bs, cs, xs = synth.planted_scenarios(3, m, n, K)
    assert np.array_equal(A, synth.planted_lp(3, m, n)[0])
    assert len(bs) == len(cs) == len(xs) == K
    for b, c, x in zip(bs, cs, xs):
        assert np.abs(A @ x - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
        basis = x > 0
        assert basis.sum() == m and x[basis].min() >= 1.0
        y = np.linalg.lstsq(A[:, basis].T, c[basis], rcond=None)[0]     # c_B = A_B^T y*  (z* = 0 on the basis)
        z = c - A.T @ y
        assert np.abs(z[basis]).max() <= 1e-9 and z[~basis].min() >= 1.0 - 1e-9
    assert not np.array_equal(bs[0], bs[1])                         # the scenarios differ

"""Build-time properties of the passes over a shared constraint matrix (kernels_gemv.hip, *_shared_kernel): every
instantiation exists and carries NO VGPR / SGPR spill and no scratch -- a group of members is held in registers, and a
spill would put a scratch round trip into every step of a pass that exists to save memory traffic.  Read from hipcc's own
resource-usage remarks; no GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_matrix_kernels_have_no_spills():
    src = os.path.join(ROOT, "lp_amd", "csrc", "kernels_gemv.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull],
                         capture_output=True, text=True, cwd=os.path.dirname(src)).stderr
    blocks = re.split(r"remark: Function Name: ", out)
    names = {"gemv_n_shared_kernel": 4, "gemv_t_shared_kernel": 2, "gemv_dual_shared_kernel": 2}
    for name, count in names.items():
        found = [b for b in blocks[1:] if name in b.splitlines()[0]]
        assert len(found) == count, (name, [b.splitlines()[0] for b in blocks[1:]])
        for b in found:
            get = lambda key: int(re.search(key + r": (\d+)", b).group(1))
            assert get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, b


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

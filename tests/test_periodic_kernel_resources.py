"""The kernels of the periodic-driving pass (periodic_batch.hip, ffk_periodic_dev / ffk_resident_periodic) keep nothing
in private memory and spill no register -- read from libffk.so as test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

# one instance per dimension: the template argument is part of the mangled name
PERIODIC = tuple(f'periodic_{kind}_kernelILi{d}E' for kind in ('fejer', 'decay') for d in (2, 3, 4))


@pytest.mark.parametrize('fragment', PERIODIC)
def test_periodic_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert len(found) == 1, (fragment, sorted(found))
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name


def test_periodic_kernels_fit_a_block_of_four_wavefronts(kernels):  # noqa: F811
    """Four wavefronts per block, one per SIMD: each within the 512 registers of a SIMD lane, the static LDS within
    the 64 KiB of a block (d = 4 decay: the rotated basis, one step of Y, the four wavefronts' tiles)."""
    for fragment in PERIODIC:
        k = [k for name, k in kernels.items() if fragment in name][0]
        assert k['.vgpr_count'] <= 512, fragment
        assert k['.group_segment_fixed_size'] <= 64*1024, fragment

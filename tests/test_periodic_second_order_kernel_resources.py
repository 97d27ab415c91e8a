"""The kernels of the second-order periodic-driving pass (periodic_batch.hip, ffk_periodic_shifts_dev /
ffk_resident_periodic_shifts) keep nothing in private memory and spill no register -- read from libffk.so as
test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

# one instance per dimension: the template argument is part of the mangled name
SHIFTS = tuple(f'periodic_shift_{kind}_kernelILi{d}E' for kind in ('gram', 'combine') for d in (2, 3, 4))


@pytest.mark.parametrize('fragment', SHIFTS)
def test_shift_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert len(found) == 1, (fragment, sorted(found))
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name


def test_shift_kernels_fit_a_block_of_four_wavefronts(kernels):  # noqa: F811
    """Four wavefronts per block, one per SIMD: each within the 512 registers of a SIMD lane, the static LDS within
    the 64 KiB of a block (d = 4 Gram: the rotated basis, one step of both operands -- whose LDS the four wavefronts'
    tiles reuse --, M and M E)."""
    for fragment in SHIFTS:
        k = [k for name, k in kernels.items() if fragment in name][0]
        assert k['.vgpr_count'] <= 512, fragment
        assert k['.group_segment_fixed_size'] <= 64*1024, fragment

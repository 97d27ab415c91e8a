"""The kernels of the batched gradient pass (grad_batch.hip, ffk_batch_filter_function_derivative) keep nothing in
private memory and spill no register -- read from libffk.so as test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

SMALL = ('gradb_prologue_kernel', 'gradb_totals_kernel', 'gradb_prefix_kernel', 'gradb_reduce_kernel')


def test_the_fused_kernel_has_three_instantiations_without_private_memory(kernels):  # noqa: F811
    """grad_batch_kernel<D> for D = 2, 3, 4: the running sums and the conjugate total of one noise operator stay in
    registers (2 d^2 complex numbers, 128 registers at d = 4), the integrals and W_a in per-lane LDS columns."""
    found = {name: k for name, k in kernels.items() if 'grad_batch_kernel' in name}
    assert len(found) == 3, sorted(found)
    for D in (2, 3, 4):
        assert sum(f'ILi{D}E' in name for name in found) == 1, (D, sorted(found))
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] == 64, name
        # one wavefront's share of the register file (d = 4 runs one wavefront per SIMD: its 33 KiB of LDS columns
        # leave room for four blocks per CU anyway)
        assert k['.vgpr_count'] + k['.agpr_count'] <= 512, (name, k['.vgpr_count'], k['.agpr_count'])


@pytest.mark.parametrize('fragment', SMALL)
def test_the_small_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert found, fragment
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name

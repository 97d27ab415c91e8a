"""The kernels of the batched processes pass (processes.hip, ffk_resident_batch_processes) keep nothing in private
memory and spill no register -- read from libffk.so as test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

PROCESSES = ('processes_decay_kernel', 'processes_reduce_kernel', 'processes_expm_kernel')


@pytest.mark.parametrize('fragment', PROCESSES)
def test_processes_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert found, fragment
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name


def test_every_instantiation_of_the_decay_kernel_is_there(kernels):  # noqa: F811
    """Real weights, complex weights, operator pairs: three instantiations.  The one for real weights is the hot
    path: 64 pulses of config 2 give 3072 wavefronts, three per SIMD, each with 8 KiB of reads in flight, so it
    must leave room for three wavefronts per SIMD (512 registers / 3, in granules of 8: 168)."""
    found = {name: k for name, k in kernels.items() if 'processes_decay_kernel' in name}
    assert len(found) == 3, sorted(found)
    real = [k for name, k in found.items() if 'ILb1ELb0E' in name]
    assert len(real) == 1
    assert real[0]['.vgpr_count'] <= 168, real[0]['.vgpr_count']
    for name, k in found.items():
        assert k['.group_segment_fixed_size'] <= 4096, (name, k['.group_segment_fixed_size'])

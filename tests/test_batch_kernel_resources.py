"""The batched kernels (ffk_pipeline_batch_dev) obey the budget of the small kernels of a pass stated in
test_kernel_resources.py -- read from libffk.so the same way (CPU test) -- and keep nothing in private memory."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

BATCH = ('eigh_expm_controls_pulses_kernel', 'scan_local_pulses_kernel', 'apply_prologue_pulses_kernel',
         'expand_ff_pulses_kernel', 'infid_pulses_kernel', 'count_failures_pulses_kernel',
         'assemble_hamiltonians_pulses_kernel')


@pytest.mark.parametrize('fragment', BATCH)
def test_batched_kernels_fit_the_small_kernel_budget(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert found, fragment
    for name, k in found.items():
        if not ('apply_prologue' in name and 'ILi16E' in name):     # (as the single-pulse kernel of d = 16)
            assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name
        if 'ILi4E' in name or 'ILi' not in name:    # the d = 4 instantiations and the untemplated kernels
            assert k['.vgpr_count'] <= 56, (name, k['.vgpr_count'])
            assert k['.group_segment_fixed_size'] <= 8192, (name, k['.group_segment_fixed_size'])

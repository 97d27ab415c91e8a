"""The instruction order of the d = 4 accumulate kernel's generated consumer loop (filter_functions_amd/csrc/
ctrl_pq_consumer.inc, tools/gen_pq_consumer.py), read from the committed file (CPU test).

Why (profiles/r06_b_*): an LDS read issued behind a matrix instruction costs the wavefront
0.5 cycles at one per two gaps and 4 at one per gap, in bursts up to 7.3; a vector FP64 instruction between two
matrix instructions costs about three times its grouped price.  So every LDS operation of the tile loop sits in a
gap behind a matrix instruction, no gap takes more than the register plan forces, a set's FP64 vector work stays
in one group in front of its matrix instructions, and the tile's LDS traffic is what it was."""
import os
import re

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, 'filter_functions_amd', 'csrc', 'ctrl_pq_consumer.inc')
RING = 8
# LDS operations per gap the generator may deal: 7 / 16 in 9 gaps (NC = 3), 7 / 12 in 6 (NC = 2), 7 / 8 in 3 (NC = 1)
MAX_PER_GAP = {1: 3, 2: 2, 3: 2}


def _loop_lines(nc):
    """the instructions of PqConsumer<nc>'s loop block, from the first slot to the exit"""
    text = open(INC).read()
    start = text.index(f'struct PqConsumer<{nc}>')
    end = text.index('struct PqConsumer<', start + 1) if nc < 3 else len(text)
    body = text[start:end]
    lines = [m.group(1).strip() for m in re.finditer(r'^\s*"(.*?)\\n\\t"', body, re.M)]
    first = lines.index('L_slot0_%=:')
    last = lines.index('L_exit%=:')
    return lines[first:last]


def _slots(nc):
    lines = _loop_lines(nc)
    heads = [i for i, ln in enumerate(lines) if re.match(r'L_slot\d_%=:', ln)]
    assert len(heads) == RING
    return [lines[a:b] for a, b in zip(heads, heads[1:] + [len(lines)])]


def _is_mfma(ln):
    return ln.startswith('v_mfma')


def _is_fp64_vector(ln):
    return re.match(r'v_\w+_f64\b', ln) is not None and not _is_mfma(ln)


@pytest.mark.parametrize('nc', [1, 2, 3])
def test_lds_operations_sit_in_matrix_gaps(nc):
    for k, slot in enumerate(_slots(nc)):
        last = None             # the last matrix / FP64 vector instruction seen
        in_gap = 0
        for ln in slot:
            if _is_mfma(ln):
                last, in_gap = 'mfma', 0
            elif _is_fp64_vector(ln):
                last, in_gap = 'valu', 0
            elif ln.startswith('ds_'):
                assert last == 'mfma', f'NC = {nc}, slot {k}: {ln!r} is not behind a matrix instruction'
                in_gap += 1
                assert in_gap <= MAX_PER_GAP[nc], f'NC = {nc}, slot {k}: {in_gap} LDS operations in one gap'


@pytest.mark.parametrize('nc', [1, 2, 3])
def test_fp64_vector_work_is_not_dealt_between_matrix_instructions(nc):
    for k, slot in enumerate(_slots(nc)):
        kinds = [('m' if _is_mfma(ln) else 'v') for ln in slot if _is_mfma(ln) or _is_fp64_vector(ln)]
        runs = re.findall(r'm+', ''.join(kinds))
        # two sets per tile, each 3 NC matrix instructions in one run
        assert [len(r) for r in runs] == [3*nc, 3*nc], f'NC = {nc}, slot {k}: matrix runs {[len(r) for r in runs]}'


@pytest.mark.parametrize('nc', [1, 2, 3])
def test_lds_operations_per_tile(nc):
    """per tile: set 1's psi, q01, q23, the flag and the partner's progress, the done counter and the own progress,
    the next tile's 4 NC W reads, T, psi, q01, q23 -- the same as before the reads moved into the gaps"""
    for k, slot in enumerate(_slots(nc)):
        ops = [ln.split()[0] for ln in slot if ln.startswith('ds_')]
        assert ops.count('ds_read_b128') == 4*nc + 4 + 3, (nc, k, ops)
        assert ops.count('ds_read_b32') == 2 and ops.count('ds_add_u32') == 1 and ops.count('ds_write_b32') == 1
        assert len(ops) == 4*nc + 11

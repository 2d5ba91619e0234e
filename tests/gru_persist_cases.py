"""The frame-level BiGRU as ONE persistent launch (csrc/gru_persist.hip): case lists over the whole range of plan(), the host
function that picks the forward instance bigru_persist_fwd_kernel<NKB, TWC> (NKB = h / 32 in {2, 4, 8, 16}, TWC in {1, 2, 4})
and deals the 16-row tiles of every (type, direction) group to chunks and waves. Shared by tests/test_gru_persist_cpu.py (the
library's launch-free report, twog_bigru_persistent_plan at 256 compute units, against what every case claims; the specification
in fp32 against fp64) and tests/test_gru_persist_gpu.py (the launches against both).

A case is a recurrence case of tests/gru_cases.py (same input recipe, same rec_inputs / rec_run: the ids are registered in
gru_cases.REC_BY_ID, not in REC_ALL) with three claims the report must confirm ON THE DEVICE THAT RUNS IT:
    inst    (NKB, TWC) of the forward instance,
    chunks  {(tiles of a chunk, tiles per wave): how many (group, chunk) combinations} -- the whole partition as a multiset,
    bwd     whether the persistent backward serves the shape (no wave owns more than one tile).
The claims are stated for 256 compute units. If plan() changes, the claim stays and the SHAPE is changed until it holds again:
the `why` says which branch the case is there for.

DEFAULT: every wave owns at most one tile -- what the default environment launches at small batches, forward and backward.
FORCED:  TWC > 1 -- launched only under TWOG_BIGRU_PERSIST=1 ("wherever it is served"); forward only, the backward reports "not
         served" and runs per step.
REFUSED: the report says "not served"; nothing is launched."""
from tests import gru_cases as GC


def _pc(id, why, h, bs, T, Es, inst, chunks, bias=True):
    c = GC._rc('persist_' + id, why, h, bs, T, Es, bias=bias)
    c.update(inst=inst, chunks=dict(chunks), bwd=inst[1] == 1)
    return c


_ONE_ROW = 'one row: two combinations, three of the four waves of every workgroup leave at once; '
DEFAULT = [
    _pc('one_row_T1', _ONE_ROW + 'T = 1: first and last step coincide, no wait, no hand-off', 64, 1, 1, (1,), (2, 1), {(1, 1): 2}),
    _pc('one_row_T2', _ONE_ROW + 'T = 2: the only hand-off is the first and the last', 64, 1, 2, (1,), (2, 1), {(1, 1): 2}),
    _pc('one_row_T3', _ONE_ROW + 'T = 3: one middle step', 64, 1, 3, (1,), (2, 1), {(1, 1): 2}),
    _pc('h64_T33', 'T = 33: a chain long enough for a wrong step index or a stale hand-off to compound', 64, 3, 33, (2, 3, 1), (2, 1), {(1, 1): 6}),
    _pc('h128_rows63', '63 rows (E = 9), rows % 16 = 15: four chunks of one tile per direction', 128, 7, 3, (9,), (4, 1), {(1, 1): 8}),
    _pc('h256_rows63', '63 rows (E = 7), rows % 16 = 15: four chunks of one tile per direction', 256, 9, 3, (7,), (8, 1), {(1, 1): 8}),
    _pc('h256_rows65', '65 rows (E = 13): one row in the last tile', 256, 5, 3, (13,), (8, 1), {(1, 1): 10}),
    _pc('h256_rows15_33', '15 and 33 rows (E = 5, 11): rows % 16 = 15 and 1 in one launch', 256, 3, 3, (5, 11), (8, 1), {(1, 1): 8}),
    _pc('h512_four_types', 'four types at h = 512: 8 groups x 32 slices = 256 workgroups, every compute unit, no room to chunk; chunks '
        'of 1, 3, 1 and 4 tiles (3, 1, 3 and 0 waves leave at once), every row count ragged', 512, 5, 3, (2, 9, 1, 12), (16, 1),
        {(1, 1): 4, (3, 1): 2, (4, 1): 2}),
    _pc('h512_uneven_split', '14 tiles dealt 3 / 4 / 3 / 4: the uneven c * rt / chunks split', 512, 17, 3, (13,), (16, 1), {(3, 1): 4, (4, 1): 4}),
    _pc('h64_maxc', 'the MAXC = 32 bound stops the growth at 128 of 256 compute units: the forward group of the 10-tile type keeps ONE '
        'two-tile chunk among eight one-tile chunks (its reverse group five two-tile chunks)', 64, 13, 3, (3, 5, 12, 1), (2, 1),
        {(1, 1): 26, (2, 1): 6}),
    _pc('h128_16_combos', '16 combinations x 8 slices: 8 one-tile chunks per direction', 128, 25, 3, (5,), (4, 1), {(1, 1): 16}),
    _pc('h512_no_bias', 'b_hh_f = b_hh_r = None at the product shape of 8 clips: hn of the first step of each direction is exactly 0 in save',
        512, 8, 3, (2, 4, 1), (16, 1), {(1, 1): 8}, bias=False),
    _pc('h256_bs6', 'three types of 12 / 48 / 6 rows, the 48-row type in three chunks', 256, 6, 3, (2, 8, 1), (8, 1), {(1, 1): 10}),
]
_MIX2 = {(2, 1): 4, (3, 1): 13, (4, 1): 10, (5, 2): 5}
_MIX4 = {(4, 1): 2, (5, 2): 2, (6, 2): 8, (7, 2): 12, (8, 2): 6, (9, 3): 2}
FORCED = [
    _pc('i16_2_beside_one_tile', '<16, 2>: one chunk of 5 tiles dealt 2 / 2 / 1 / 0 beside one-tile chunks in the same launch',
        512, 5, 3, (1, 1, 1, 13), (16, 2), {(1, 1): 6, (5, 2): 2}),
    _pc('i16_2', '<16, 2>: chunks of 6 / 7 / 7 / 7 tiles, two per wave with a short or empty last wave', 512, 33, 3, (13,), (16, 2), {(6, 2): 2, (7, 2): 6}),
    _pc('i16_4_three_per_wave', '<16, 4>: 9 tiles dealt 3 / 3 / 3 / 0 (tw = 3 in the TWC = 4 instance) beside one-tile chunks',
        512, 10, 3, (1, 1, 1, 13), (16, 4), {(1, 1): 6, (9, 3): 2}),
    _pc('i16_4', '<16, 4>: chunks of 13 / 13 / 13 / 14 tiles, four per wave with a short last wave', 512, 65, 3, (13,), (16, 4), {(13, 4): 6, (14, 4): 2}),
    _pc('i8_2', '<8, 2>: ring depth D = 8 = NKB', 256, 65, 3, (1, 1, 1, 2), (8, 2), {(2, 1): 6, (3, 1): 6, (4, 1): 2, (5, 2): 2}),
    _pc('i8_4', '<8, 4>: ring depth D = 3, tiles per wave 1, 2 and 3', 256, 26, 3, (5, 5, 5, 11), (8, 4), {(4, 1): 6, (5, 2): 6, (9, 3): 4}),
    _pc('i4_2', '<4, 2>: ring depth D = 4 = NKB, 32 combinations', 128, 65, 3, (1, 1, 2, 9), (4, 2), _MIX2),
    _pc('i4_4', '<4, 4>: ring depth D = 3 of NKB = 4', 128, 43, 3, (3, 12, 12, 12), (4, 4), _MIX4),
    _pc('i2_2', '<2, 2>: ring depth D = 2 = NKB', 64, 65, 3, (1, 1, 2, 9), (2, 2), _MIX2),
    _pc('i2_4', '<2, 4>: D = min(NKB, 3) = 2; tiles per wave 1, 2 and 3 in one launch', 64, 43, 3, (3, 12, 12, 12), (2, 4), _MIX4),
]
LAUNCHED = DEFAULT + FORCED
GC.REC_BY_ID.update({c['id']: c for c in LAUNCHED})

N_CUS = 256   # the compute units the claims are stated for (MI355X)
# (id, why, Es, bs, h, n_cus): the report is "not served"
REFUSED = [
    ('five_types', 'more than MAXG / 2 = 4 types', (1, 1, 1, 1, 1), 3, 64, N_CUS),
    ('h96', 'hidden not 64 / 128 / 256 / 512', (2, 3, 1), 3, 96, N_CUS),
    ('empty_type', 'a type with E = 0: a group without a row tile', (2, 0, 3), 3, 64, N_CUS),
    ('chunk_of_17', 'tiles 9 / 33 / 5 in 8 combinations at h = 512: a chunk of 17 tiles, more than four per wave', (2, 8, 1), 65, 512, N_CUS),
    ('too_few_cus', '2 x 3 types x 512 / 16 = 192 workgroups on 128 compute units', (2, 3, 1), 3, 512, 128),
]

INSTANCES = {(nkb, twc) for nkb in (2, 4, 8, 16) for twc in (1, 2, 4)}   # the twelve forward instances that ship
BWD_WIDTHS = {64, 128, 256, 512}                                          # the four instances of the backward kernel
LDS_LIMIT = 160 * 1024


def type_rows(c):
    """Rows (clips x entities) of every type of case c."""
    return [c['bs'] * E for E in c['Es']]


def claimed(plan):
    """What a report (kernels.bigru_persistent_plan / _lib.bigru_persistent_plan) says in the terms of a case's claims."""
    chunks = {}
    for _, rt0, rt1, tw in plan['combos']:
        chunks[(rt1 - rt0, tw)] = chunks.get((rt1 - rt0, tw), 0) + 1
    return dict(inst=(plan['nkb'], plan['twc']), chunks=chunks, bwd=plan['bwd_served'])


def claims(c):
    return dict(inst=c['inst'], chunks=c['chunks'], bwd=c['bwd'])


def first_step_hn_rows(c, k):
    """Index of the rows of `save{k}` of rec_run ([2][bs][T][E][4h] as rows of h) that hold hn of the FIRST step of either
    direction (t = 0 forward, t = T - 1 reverse): exactly 0 where the case has no bias."""
    bs, T, E = c['bs'], c['T'], c['Es'][k]
    rows = []
    for d, t in ((0, 0), (1, T - 1)):
        for b in range(bs):
            for e in range(E):
                rows.append(((((d * bs + b) * T + t) * E + e) * 4) + 3)
    return rows

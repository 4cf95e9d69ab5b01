"""GPU parity tests (pytest -m gpu) of the implicit-GEMM convolutions (csrc/conv.hip, csrc/igemm_wide.h, csrc/igemm_nwalk.h) on exact
integer lattices: forward, data gradient and weight gradient with their epilogues -- statistics (plain, statistics-only, pivoted), the
fused BatchNorm-backward reduce in its four mask modes (store / accumulate) and the fused BatchNorm-apply tails -- called through the C
ABI and compared with float64 references at tolerance ZERO.

On small-integer operands (x, dy in [-2, 2], w in {-1, 0, 1}, thinned by the reduction length; tests/conv_reference.py) every product and
every partial sum is exactly representable in each matrix arithmetic -- bf16 storage, fp32 `exact`, bf16x3, bf16x6, bf16x6_3, f16x3_3 --
so neither the summation order, nor the split tail's exchange through its fp32 scratch, nor the weight gradient's slab sum changes a bit:
one dropped or double-counted row of a statistic, a swapped IH / IW, a wrong OW in a row decode or one wrong mask decision is a non-zero
error however many rows the layer has.  In mask mode 2 no element is exempted: the lattice makes the mask argument exact, zeros included.
Every check first asserts those conditions on the CPU (conv_reference.reference: float32 evaluation == float64 evaluation, storage
survival, magnitude bounds, non-degeneracy floors).  Operand range and the accuracy of the split pieces are NOT the subject here (the
Gaussian tests of tests/test_gpu_kernels.py measure those): geometry, row accounting and epilogue bookkeeping are.

Every output lives in a guarded buffer (gpu_checks._guarded) that starts from a sentinel; after each launch the recorded instantiation
(simclr_conv2d_last_instantiation) must name the kernel family and the template arguments the row claims -- the claims are checked
without a GPU too, in a dry run (tests/test_conv_reference.py).  Rows with statistics run with simclr_conv2d_stats_slots + 5 slots (the
five spare slots stay zero) and with 1 and 3 slots (the float-atomics branch gives the same totals).

The rows (conv_reference.build_cases): non-square maps (5x9, 9x5, 1x7, 7x1, 6x10; stride 2 on 7x10 and 10x7) in every family; row counts 1,
127 / 128 / 129, 255 / 256 / 257 (256-row tiles), 63 / 64 / 65 (N-inner walk); per persistent family the smallest row count at which a
workgroup owns several M-tiles and the last round is partial; Cout 4 ... 320, fp32 Cin 32 / 96, the BN 64 / 128 switch and the narrow-tile
rule's boundaries; halo window W = 61 / 62 / 63 and H = 1; nine-tap weight gradient W = 6 / 7; split tails on the 128-wide, the 256-wide and
the eight-phase tile; every weight-gradient family with accumulate 0 / 1 and one / several slabs; two designated bf16 rounding rows whose
outputs exceed 8 significant bits (128-wide tile: statistics of the exact accumulators; SIMCLR_IGEMM_TILE=256: of the bf16-rounded
outputs; y = the exact value rounded once in both) plus the same on the eight-phase tile.

`ext` rows: the K-extended data gradient simclr_conv2d_dgrad_ext (accumulate 0 / 1) and simclr_conv2d_dgrad_bn_ext (the four mask modes,
store and accumulate, statistics at the three slot counts) -- dm and h on the lattice, w_ext in {-1, 0, 1} thinned by Cout + Cin, an
integer bias; Cin = / < / > Cout, fp32 32 + 64 channels (no multiple of a 64-element k-tile), rows 1, 127 / 128 / 129, 255 / 256 / 257, the
128-row tile in both storage types and the SIMCLR_IGEMM_TILE=256 class in bf16; arithmetics bf16, exact, bf16x3, f16x3_3.
`sparse` rows: the 1x1 stride-2 data gradient with accumulate = 3 into a dx full of a finite sentinel (12345: even (row, column) pixels =
the reference, every other element still the sentinel; fp32 and bf16), then a stride-1 data gradient (plain, and with the fused reduce
in mask modes 2 and 4) with accumulate = 2 into what that call left: second + first at the even pixels, second alone elsewhere -- a
leaked sentinel is a wrong number, not a masked compare; maps 7x10, 10x7, 1x9, 9x1 and rows 1, 127 / 128 / 129, channels 32 <-> 64.
The stem chain and the Gram chain have their own module, tests/test_gpu_stem_gram_lattice.py.

Left out: the TILE256_BF16 weight gradient (no forcing switch: it needs M >= 150000); the persistent-loop tail of the stem forward (more
than 2048 M-tiles need 306 456 rows: tests/test_gpu_kernels.py covers it with Gaussian inputs); the K-extended launch on a pre-split dm
(plan_igemm has no such kernel and refuses it).  The non-persistent fallback kernel adds its statistics with float atomics into slot (M-tile % nslot)
whatever the slot count, so "spare slots stay zero" holds for it only because its rows here have a single M-tile."""
import pytest

from tests.conv_reference import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _exact_f32_matmul():
    """simclr_set_f32_matmul is process-wide: every test starts (and leaves) the library in the exact fp32 mode."""
    from simclr_amd import ops
    ops.set_f32_matmul('exact')
    yield
    ops.set_f32_matmul('exact')


def _assert(results):
    bad = [r for r in results if not r['ok']]
    for r in bad:
        print('FAIL %-90s err=%.3e nbad=%d of %d' % (r['name'], r['err'], r.get('nbad', 0), r.get('numel', 0)))
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_conv_lattice_bitwise(case):
    from tests import gpu_checks as gc
    _assert(gc.check_conv_lattice(case))

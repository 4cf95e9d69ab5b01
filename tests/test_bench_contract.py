"""bench.py pieces that can be checked without a GPU: the roofline entry follows the contract
({bound, achieved, peak, unit, frac, traffic}) and picks the binding roof from the arithmetic intensity."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_roofline_entry_memory_bound_family():
    b = _bench()
    # 100 launches, 160 FLOP/B: below the bf16 ridge (2500e12 / 8000e9 = 312.5) -> HBM is the binding roof
    r = b.make_roofline('conv_igemm', flops=100 * 1.6e11, min_bytes=100 * 1.0e9, impl_bytes=100 * 1.2e9, total_ms=100 * 0.4,
                        launches=100, steps=2, mfma_peak_tflops=2500.0)
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0
    assert abs(r['achieved'] - 2500.0) < 1e-6 and abs(r['frac'] - 2500.0 / 8000.0) < 1e-4      # from the MINIMUM bytes
    assert abs(r['impl_gbps'] - 3000.0) < 1e-6 and r['impl_bytes_per_launch'] == 1_200_000_000
    assert r['traffic'] is None and r['launches_per_step'] == 50
    assert abs(r['achieved_tflops'] - 400.0) < 1e-6 and abs(r['mfma_frac'] - 0.16) < 1e-4
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r
    # the strict SURVEY 8(d) fraction beside the one that counts the fused-epilogue operands, and an
    # explicit statement that `traffic` comes from the committed PMC passes, not from this run
    assert r['strict_frac'] == r['frac'] and abs(r['fused_operands_frac'] - 3000.0 / 8000.0) < 1e-4
    assert r['traffic_measured_in_run'] is False


def test_roofline_entry_compute_bound_family():
    b = _bench()
    r = b.make_roofline('conv_igemm', flops=10 * 4.0e11, min_bytes=10 * 1.0e9, impl_bytes=10 * 1.0e9, total_ms=10 * 0.5,
                        launches=10, steps=1, mfma_peak_tflops=2500.0)
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and r['peak'] == 2500.0
    assert abs(r['achieved'] - 800.0) < 1e-6 and abs(r['frac'] - 0.32) < 1e-4 and r['traffic'] is None


def test_step_time_percentiles_and_self_launch_command():
    b = _bench()
    p = b.percentiles([float(i) for i in range(1, 102)])
    assert p == dict(p10=11.0, median=51.0, p90=91.0, n=101)
    # `python bench.py --gpus N` without a torchrun environment re-launches itself with one rank per GPU
    import inspect
    src = inspect.getsource(b.relaunch_multi_gpu)
    for needle in ('torch.distributed.run', '--nproc-per-node', '--master-addr', '127.0.0.1'):
        assert needle in src


def test_flop_table_and_backend_flag():
    """cfg4 / cfg5 carry their own FLOP-per-image constants, so `step_mfma_frac` is never null for them; the
    gloo backend switch exists for exercising the N > 1 path on one GPU."""
    b = _bench()
    assert b.FLOP_PER_IMAGE_BY_MODEL[(50, 1, False)] == b.FLOP_PER_IMAGE == 49.15e9
    assert b.FLOP_PER_IMAGE_BY_MODEL[(50, 2, True)] == 296.6e9 and b.FLOP_PER_IMAGE_BY_MODEL[(152, 3, True)] == 1893.6e9
    import inspect
    src = inspect.getsource(b.main)
    for needle in ("'--backend'", 'SIMCLR_DIST_BACKEND', 'SIMCLR_SHARE_GPU', 'peak_hbm_gb', 'stat_collectives_per_step'):
        assert needle in src, needle


def test_parity_block_is_measured_not_claimed():
    """VERDICT r04 / ADVICE r04: the line's `parity` object is computed in the run from the reference-source fixtures -- no hard-coded
    claim survives in bench.py, the inputs come from tests/golden/recipe.py (pure numpy, no oracle import outside cpu_baseline)."""
    import inspect
    import re
    b = _bench()
    src = open(os.path.join(ROOT, 'bench.py')).read()
    assert 'north_star met' not in src and 'PARITY_NOTE' not in src
    msrc = inspect.getsource(b.measured_parity)
    for needle in ('measured_in_run', 'reference_pin.npz', 'recipe.variable_value', 'make_single_step', 'north_star_met'):
        assert needle in msrc, needle
    assert 'oracle' not in re.sub(r'""".*?"""', '', msrc, flags=re.S).replace("oracle/tfshim.py", '')      # the docstring may name it
    # only the cpu_baseline leg imports the oracle
    body = src.replace(inspect.getsource(b.cpu_baseline), '')
    assert 'from oracle' not in body and 'import oracle' not in body
    # the recipe really is oracle-free and deterministic by NAME
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location('recipe', os.path.join(ROOT, 'tests', 'golden', 'recipe.py'))
    r = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(r)
    rsrc = open(os.path.join(ROOT, 'tests', 'golden', 'recipe.py')).read()
    assert 'import torch' not in rsrc and 'from oracle' not in rsrc
    a = r.variable_value('resnet/conv2d_fixed_padding/conv2d/kernel:0', np.zeros((3, 3, 3, 8)), True)
    assert np.array_equal(a, r.variable_value('resnet/conv2d_fixed_padding/conv2d/kernel:0', np.ones((3, 3, 3, 8)), False))
    assert np.abs(a).max() <= 2 * (1 / 27) ** 0.5 / .87962566103423978 + 1e-12
    g = r.variable_value('x/gamma:0', np.ones(4), True)
    assert np.all((g >= 1.5) & (g < 2.5)) and np.array_equal(r.variable_value('x/gamma:0', np.ones(4), False), np.ones(4))
    assert set(r.IMG_CASES) == {'r18_img', 'r50_img'}


def test_parity_mode_and_ntxent_accounting_fields():
    import inspect
    b = _bench()
    src = inspect.getsource(b.main)
    for needle in ('split_roofline', "'families'", 'mfma_terms', 'traffic_measured_in_run', "kernels=7", 'us_events_in_step',
                   'rccl_ranks_seen', 'rank_devices', 'stat_transport'):
        assert needle in src, needle
    csrc = inspect.getsource(b.cpu_baseline)
    assert 'warm=3' in csrc and 'min_steps=10' in csrc


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: what the last timed step handed its caller, as float32 .npy files; an output of more than DUMP_SAMPLE elements
    becomes the same sorted sample of its elements in every run, and the whole dump stays under 64 MB."""
    import inspect
    import types
    import numpy as np
    import torch
    b = _bench()
    src = inspect.getsource(b.main)
    for needle in ("'--dump-outputs'", 'last = step_fn(f, l)', 'dump_outputs(args.dump_outputs, last, model)'):
        assert needle in src, needle
    # the dump is taken before the instrumented steps, which would move the variables and gradients past the last timed step
    assert src.index('dump_outputs(args.dump_outputs') < src.index('prof = ops.KernelProfiler()')
    n = b.DUMP_SAMPLE // 2 + 1000                   # two trainable tensors of n elements + one statistic: both big arrays get sampled
    ns = types.SimpleNamespace
    w = [ns(value=torch.arange(i * n, (i + 1) * n, dtype=torch.float32), grad=torch.arange(i * n, (i + 1) * n, dtype=torch.float32))
         for i in range(2)]
    stat = ns(value=torch.arange(2 * n, 2 * n + 64, dtype=torch.float32))
    model = ns(variables=w + [stat], trainable_variables=w)
    one = lambda x: torch.tensor([x])
    emb = torch.randn(16, 4)
    out = dict(con_loss=ns(value=one(2.5), normalized=emb), logits_con=ns(contrast_acc=one(0.25), contrast_entropy=one(1.5)),
               sup_loss=ns(value=one(6.9), acc=one(0.0)), weight_decay=one(1e-3), total_loss=one(9.401))
    b.dump_outputs(str(tmp_path / 'a'), out, model)
    b.dump_outputs(str(tmp_path / 'b'), out, model)
    names = {'contrast_loss', 'contrast_acc', 'contrast_entropy', 'supervised_loss', 'supervised_acc', 'weight_decay', 'total_loss',
             'embeddings', 'variables', 'gradients'}
    assert {p.name for p in (tmp_path / 'a').iterdir()} == {x + '.npy' for x in names}
    got = {x: np.load(tmp_path / 'a' / (x + '.npy')) for x in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(os.path.getsize(tmp_path / 'a' / (x + '.npy')) for x in names) <= 64 << 20
    assert got['total_loss'].tolist() == [np.float32(9.401)] and np.array_equal(got['embeddings'], emb.numpy())
    for x, total in (('variables', 2 * n + 64), ('gradients', 2 * n)):
        s = got[x]
        # element values equal their positions here: a sorted sample of distinct elements of the concatenation
        assert s.shape == (b.DUMP_SAMPLE,) and np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < total
        assert np.array_equal(s, np.load(tmp_path / 'b' / (x + '.npy')))


def test_headline_is_the_tolerance_meeting_mode():
    """with no flags the top-level value / dtype / roofline of the line belong to the fastest mode that meets
    north_star's tolerances (fp32 storage, three fp16-piece terms forward, three bf16-piece terms backward); the bf16 speed mode is a
    `speed_mode` sub-block, and the line says whether its own in-run parity measurement met the tolerances."""
    import inspect
    import re
    b = _bench()
    src = inspect.getsource(b.main)
    assert re.search(r"'--dtype', default='f32'", src) and re.search(r"'--f32_matmul', default='f16x3_3'", src)
    for needle in ("'speed_mode'", "'north_star_met'", "'f32_mode'", "'parity_mode_bf16x6'", "'dtype_detail'"):
        assert needle in src, needle
    from simclr_amd import ops
    assert ops.F32_MATMUL_TERMS['f16x3_3'] == (13, 3)

"""The table of pretraining losses (simclr_amd/pretrain_losses.py) as run.py reads it: one predicate, the metric names of every loss,
and the start-up width check of every loss -- no GPU."""
import pytest

from simclr_amd import model as model_lib
from simclr_amd import pretrain_losses, run
from simclr_amd.flags import FLAGS

NAMES = ['ntxent', 'generalized', 'supcon', 'barlow', 'vicreg', 'byol', 'mocov2', 'dino', 'swav']

RUN_PREDICATES = {'generalized': run.generalized_loss_on, 'supcon': run.supcon_loss_on, 'barlow': run.barlow_loss_on,
                  'vicreg': run.vicreg_loss_on, 'byol': run.byol_loss_on, 'mocov2': run.moco_loss_on, 'dino': run.dino_loss_on,
                  'swav': run.swav_loss_on}
MODEL_PREDICATES = {'byol': model_lib.byol_on, 'mocov2': model_lib.moco_on, 'dino': model_lib.dino_on, 'swav': model_lib.swav_on}

SUPERVISED = ['train/supervised_acc', 'train/supervised_loss']
COMMON = ['train/total_loss', 'train/weight_decay']
# written out from the table of the losses: every loss logs train/contrast_loss, then its own terms
LOSS_METRICS = {
    'ntxent': ['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_loss'],
    'generalized': ['train/align_loss', 'train/contrast_loss', 'train/dist_loss'],
    'supcon': ['train/contrast_acc', 'train/contrast_loss', 'train/contrast_positives'],
    'barlow': ['train/bt_off_diag', 'train/bt_on_diag', 'train/contrast_loss'],
    'vicreg': ['train/contrast_loss', 'train/vicreg_cov', 'train/vicreg_inv', 'train/vicreg_var'],
    'byol': ['train/byol_cosine', 'train/contrast_loss'],
    'mocov2': ['train/contrast_acc', 'train/contrast_loss'],
    'dino': ['train/contrast_loss', 'train/dino_teacher_entropy'],
    'swav': ['train/contrast_loss', 'train/swav_code_entropy'],
}

# --proj_out_dim=100 under the default flags: the message check_contrastive_loss_flags raised before the table existed, verbatim
GOT = "(got proj_head_mode='nonlinear', proj_out_dim=100)"
FROM = "(got 100 from proj_head_mode='nonlinear', proj_out_dim=100)"
WIDTH_MESSAGES = {
    'generalized': "--contrastive_loss=generalized needs a projection head of width 64/128/256 " + GOT
                   + ": the generalized-loss kernels are instantiated for those widths only",
    'supcon': "--contrastive_loss=supcon needs a projection head of width 64/128/256 " + GOT
              + ": the supervised contrastive kernels are instantiated for those widths only",
    'barlow': "--contrastive_loss=barlow needs a loss width that is a multiple of 64 in [64, 8192] " + FROM
              + ": the Barlow Twins kernels take those widths only",
    'vicreg': "--contrastive_loss=vicreg needs a loss width that is a multiple of 64 in [64, 8192] " + FROM
              + ": the VICReg kernels take those widths only",
    'byol': "--contrastive_loss=byol needs a loss width that is a multiple of 64 in [64, 8192] " + FROM
            + ": the BYOL kernels and the predictor take those widths only",
    'mocov2': "--contrastive_loss=mocov2 needs a projection head of width 64/128/256 " + GOT
              + ": the MoCo kernels are instantiated for those widths only",
    'dino': "--contrastive_loss=dino needs a projection head of width 64/128/256 " + GOT
            + ": the DINO kernels are instantiated for those widths only",
    'swav': "--contrastive_loss=swav needs a projection head of width 64/128/256 " + GOT
            + ": the SwAV kernels are instantiated for those widths only",
}


@pytest.fixture(autouse=True)
def _default_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def test_the_table_has_one_row_per_loss_name():
    assert sorted(pretrain_losses.LOSSES) == sorted(NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_exactly_the_matching_predicate_is_true(name):
    FLAGS.update(contrastive_loss=name)
    assert model_lib.pretrain_loss() == name
    assert {n for n, on in RUN_PREDICATES.items() if on()} == ({name} - {'ntxent'})
    for n, on in MODEL_PREDICATES.items():
        assert on() is RUN_PREDICATES[n]() is (n == name)
    FLAGS.update(train_mode='finetune')                                  # fine-tuning has no contrastive loss and ignores the flag
    assert model_lib.pretrain_loss() is None and pretrain_losses.active() is None
    assert not any(on() for on in RUN_PREDICATES.values()) and not any(on() for on in MODEL_PREDICATES.values())
    assert run.check_contrastive_loss_flags() is False


@pytest.mark.parametrize('name', NAMES)
def test_build_metrics_lists_the_names_of_the_row(name):
    FLAGS.update(contrastive_loss=name)
    assert sorted(run.build_metrics()) == sorted(LOSS_METRICS[name] + SUPERVISED + COMMON)       # lineareval_while_pretraining
    FLAGS.update(lineareval_while_pretraining=False)
    assert sorted(run.build_metrics()) == sorted(LOSS_METRICS[name] + COMMON)
    assert [n for n, _ in pretrain_losses.LOSSES[name].metrics][0] == 'train/contrast_loss'
    FLAGS.update(lineareval_while_pretraining=True, train_mode='finetune')
    assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
    FLAGS.update(teacher_checkpoint='/some/teacher')
    assert sorted(run.build_metrics()) == ['train/distill_agreement', 'train/distill_loss', 'train/total_loss', 'train/weight_decay']


def test_no_metric_set_exceeds_the_bank():
    for name in NAMES:
        FLAGS.reset()
        FLAGS.update(contrastive_loss=name)
        assert len(run.build_metrics()) <= 16                            # simclr_accumulate_scalars: 16 running sums


@pytest.mark.parametrize('name', sorted(WIDTH_MESSAGES))
def test_an_out_of_range_width_is_refused_in_the_words_of_its_loss(name):
    FLAGS.update(contrastive_loss=name, proj_out_dim=100)
    with pytest.raises(ValueError) as e:
        run.check_contrastive_loss_flags()
    assert str(e.value) == WIDTH_MESSAGES[name]
    FLAGS.update(mode='eval')                                            # evaluation trains no loss: nothing to refuse
    assert run.check_contrastive_loss_flags() is False


def test_ntxent_takes_any_width_and_only_the_generalized_loss_returns_true():
    FLAGS.update(contrastive_loss='ntxent', proj_out_dim=100)
    assert run.check_contrastive_loss_flags() is False
    for name in NAMES:
        FLAGS.reset()
        FLAGS.update(contrastive_loss=name, proj_out_dim=64, moco_queue_size=2 * FLAGS.train_batch_size)
        assert run.check_contrastive_loss_flags() is (name == 'generalized')

"""absl.flags-compatible shim carrying every flag of /root/reference/tf2/run.py:37-238.

The reference reads a global `FLAGS` inside library code (tf2/resnet.py:50,56,...;
tf2/model.py:31-41,...).  absl is not installed here, so this module provides the same
spellings, defaults and `--name=value` / `--noname` command-line syntax behind a
module-level `FLAGS` namespace.  TPU flags are accepted and ignored.
"""
import argparse
import collections
import contextlib

# The product default of f32_matmul is the fast tolerance-meeting mode.  SIMCLR_DEFAULT_F32_MATMUL overrides the DEFAULT only (tests/conftest.py
# sets it to 'exact': the test-suite pins the arithmetic it tests explicitly and calibrated its fp32 gates on the exact fp32-input MFMA).
_F32_MATMUL_DEFAULT = __import__('os').environ.get('SIMCLR_DEFAULT_F32_MATMUL', 'f16x3_3')

_DEFS = [
    # (name, default, type, help)                                      tf2/run.py line
    ('learning_rate', 0.3, float, 'Initial learning rate per batch size of 256.'),      # :37
    ('learning_rate_scaling', 'linear', str, "How to scale the learning rate: 'linear' or 'sqrt'."),  # :41
    ('warmup_epochs', 10, float, 'Number of epochs of warmup.'),                         # :45
    ('weight_decay', 1e-6, float, 'Amount of weight decay to use.'),                     # :49
    ('batch_norm_decay', 0.9, float, 'Batch norm decay parameter.'),                     # :51
    ('train_batch_size', 512, int, 'Batch size for training.'),                          # :55
    ('train_split', 'train', str, 'Split for training.'),                                # :59
    ('train_epochs', 100, int, 'Number of epochs to train for.'),                        # :63
    ('train_steps', 0, int, 'Number of steps to train for. If provided, overrides train_epochs.'),  # :67
    ('eval_steps', 0, int, 'Number of steps to eval for.'),                              # :71
    ('eval_batch_size', 256, int, 'Batch size for eval.'),                               # :75
    ('checkpoint_epochs', 1, int, 'Number of epochs between checkpoints/summaries.'),    # :79
    ('checkpoint_steps', 0, int, 'Number of steps between checkpoints/summaries.'),      # :83
    ('eval_split', 'validation', str, 'Split for evaluation.'),                          # :88
    ('dataset', 'imagenet2012', str, 'Name of a dataset.'),                              # :92
    ('cache_dataset', False, bool, 'Whether to cache the entire dataset in memory.'),    # :96
    ('mode', 'train', str, "'train', 'eval' or 'train_then_eval'."),                     # :102
    ('train_mode', 'pretrain', str, "'pretrain' or 'finetune'."),                        # :106
    ('lineareval_while_pretraining', True, bool, 'Whether to finetune supervised head while pretraining.'),  # :110
    ('checkpoint', None, str, 'Loading from the given checkpoint for fine-tuning.'),     # :113
    ('zero_init_logits_layer', False, bool, 'If True, zero initialize layers after avg_pool.'),  # :118
    ('fine_tune_after_block', -1, int, 'Layers after this block are fine-tuned.'),       # :122
    ('master', None, str, 'Address/name of the TensorFlow master (ignored).'),           # :128
    ('model_dir', None, str, 'Model directory for training.'),                           # :133
    ('data_dir', None, str, 'Directory where dataset is stored.'),                       # :137
    ('use_tpu', True, bool, 'Ignored (MI355X build).'),                                  # :141
    ('tpu_name', None, str, 'Ignored.'),                                                 # :145
    ('tpu_zone', None, str, 'Ignored.'),                                                 # :151
    ('gcp_project', None, str, 'Ignored.'),                                              # :157
    ('optimizer', 'lars', str, "'momentum', 'adam' or 'lars'."),                         # :163
    ('momentum', 0.9, float, 'Momentum parameter.'),                                     # :167
    ('eval_name', None, str, 'Name for eval.'),                                          # :171
    ('keep_checkpoint_max', 5, int, 'Maximum number of checkpoints to keep.'),           # :175
    ('keep_hub_module_max', 1, int, 'Maximum number of Hub modules to keep.'),           # :179
    ('temperature', 0.1, float, 'Temperature parameter for contrastive loss.'),          # :183
    ('hidden_norm', True, bool, 'Temperature parameter for contrastive loss.'),          # :187
    ('proj_head_mode', 'nonlinear', str, "'none', 'linear', 'nonlinear'."),              # :191
    ('proj_out_dim', 128, int, 'Number of head projection dimension.  MI355X build: any width; up to 256 the contrastive loss runs '
                               'the register-resident NT-Xent sweeps, wider embeddings (and proj_head_mode=none, which feeds the '
                               "encoder's 512 ... 8192-wide output) the tiled wide NT-Xent kernels."),     # :195
    ('num_proj_layers', 3, int, 'Number of non-linear head layers.'),                    # :199
    ('ft_proj_selector', 0, int, 'Which layer of the projection head to use during fine-tuning.'),  # :203
    ('global_bn', True, bool, 'Whether to aggregate BN statistics across distributed cores.'),  # :208
    ('width_multiplier', 1, int, 'Multiplier to change width of network.'),              # :212
    ('resnet_depth', 50, int, 'Depth of ResNet.'),                                       # :216
    ('sk_ratio', 0., float, 'If it is bigger than 0, it will enable SK.'),               # :220
    ('se_ratio', 0., float, 'If it is bigger than 0, it will enable SE.'),               # :224
    ('image_size', 224, int, 'Input image size.'),                                       # :228
    ('color_jitter_strength', 1.0, float, 'The strength of color jittering.'),           # :232
    ('use_blur', True, bool, 'Whether or not to use Gaussian blur for augmentation during pretraining.'),  # :236
    # build-specific (not in the reference)
    # Defaults (round 6): the mode whose outputs meet north_star's tolerances against the reference TF2 path (loss 1e-3 relative, normalised
    # embeddings 1e-5 absolute) -- fp32 storage, three fp16-piece MFMA terms forward, three bf16-piece terms backward.  --compute_dtype=bf16
    # is the opt-in speed mode: bf16 storage is narrower than the reference's fp32 and misses those tolerances (4.5e-3 / 2.3e-2 measured).
    ('compute_dtype', 'f32', str, "MI355X build: activation/compute dtype, 'f32' (parity, default) or 'bf16' (speed; narrower than the reference)."),
    ('f32_matmul', _F32_MATMUL_DEFAULT, str, "MI355X build, compute_dtype='f32' only: matrix arithmetic of the fp32 convolutions / dense layers. "
                                  "'exact' = fp32-input MFMA (1/16 of the bf16 rate); 'bf16x3' / 'bf16x6' = every fp32 product as 3 / 6 "
                                  "bf16 MFMA terms with fp32 accumulation (fp32 storage everywhere); 'bf16x6_3' = 6 terms forward, 3 "
                                  "backward (forward at fp32 level, gradients at ~2^-17); 'f16x3_3' = 3 split-FP16 terms forward (11-bit pieces: ~2^-22 per "
                                  "product at half the MFMA work of six bf16 terms), 3 bf16 terms backward -- the fast parity mode.  Ignored (exact) when "
                                  "compute_dtype='bf16': fp32 heads on a bf16 encoder always run the exact fp32-input MFMA."),
    ('ntxent_matmul', 'exact', str, "MI355X build: matrix arithmetic of the fused NT-Xent sweeps: 'exact' = fp32-input MFMA (default); 'f16x3' = "
                                     "three fp16-piece MFMA terms per product (l2-normalised hiddens lie in fp16's range; ~2^-22 / temperature on "
                                     "the logits) -- 2-3x faster at the 8-GPU shape, opt-in.  Embeddings wider than 256 (the wide NT-Xent kernels) always run "
                                     "'exact': 'f16x3' falls back to it there."),
    ('head_dtype', 'same', str, "MI355X build: dtype of the projection / supervised heads: 'same' (= compute_dtype) or 'f32' "
                                "(the heads are 0.2 % of the FLOPs; fp32 there keeps the loss gradient exact)."),
    # the input pipeline of simclr_amd/data.py (--dataset other than 'synthetic')
    ('data_seed', 0, int, 'MI355X build: seed of the per-epoch permutations and of the augmentation draws; the batch of a step depends on '
                          '(data_seed, step, replica) only, so a resumed run continues the same data.'),
    ('input_threads', 2, int, 'MI355X build: host threads that gather the records of the next batches into pinned buffers.'),
    ('prefetch_batches', 2, int, 'MI355X build: batches gathered ahead of the one the step consumes.'),
    # self-training / distillation (the third SimCLRv2 stage, tf2/colabs/distillation_self_training.ipynb): a frozen fine-tuned teacher
    # supplies the targets of the student's fine-tuning step
    ('teacher_checkpoint', None, str, 'MI355X build: checkpoint of a fine-tuned model (supervised head included).  When set, --train_mode=finetune '
                                      'distils that frozen teacher into the student: the loss of a step is add_kd_loss(student logits, teacher '
                                      'logits, distill_temperature) on the step\'s images, labels are not read.  Every teacher variable must be '
                                      'in the file with its shape.  Ignored by --mode=eval.'),
    ('distill_temperature', 1.0, float, 'MI355X build: temperature T of the distillation loss T^2 * CE(softmax(teacher / T), student / T).'),
    ('teacher_resnet_depth', None, int, "MI355X build: depth of the teacher's ResNet (default: --resnet_depth)."),
    ('teacher_width_multiplier', None, int, "MI355X build: width multiplier of the teacher (default: --width_multiplier)."),
    ('teacher_sk_ratio', None, float, "MI355X build: selective-kernel ratio of the teacher (default: --sk_ratio)."),
    ('teacher_ft_proj_selector', None, int, 'MI355X build: projection-head layer the teacher\'s supervised head reads (default: --ft_proj_selector).'),
    # generalized contrastive loss (colabs/intriguing_properties/generalized_contrastive_loss.ipynb) in place of NT-Xent for pretraining
    ('contrastive_loss', 'ntxent', str, "MI355X build: pretraining loss, 'ntxent' (add_contrastive_loss, default), 'generalized' "
                                        '(generalized_contrastive_loss: alignment + gcl_lambda x distribution matching; projection width 64, 128 or 256) '
                                        "or 'supcon' (add_supcon_loss: supervised contrastive loss, every same-class row of the global batch a positive; "
                                        "projection width 64, 128 or 256) or 'barlow' (add_barlow_twins_loss: Barlow Twins, no negatives; loss width "
                                        '= proj_out_dim, or the encoder width with proj_head_mode=none, a multiple of 64 in [64, 8192]; --hidden_norm and '
                                        "--temperature are ignored with it) or 'byol' (add_byol_loss: BYOL on a momentum target network with a predictor "
                                        'on the online side; loss width as for barlow; always l2-normalised, --hidden_norm and --temperature are ignored) '
                                        "or 'mocov2' (add_moco_loss: MoCo v2, InfoNCE against a queue of momentum keys; loss width 64, 128 or 256; always "
                                        'l2-normalised, --hidden_norm is ignored, --temperature is honoured: 0.2 is the usual choice) '
                                        "or 'dino' (add_dino_loss: DINO self-distillation onto --dino_out_dim prototypes, a momentum target network and "
                                        'a centre; loss width 64, 128 or 256; always l2-normalised, --hidden_norm and --temperature are ignored) '
                                        "or 'swav' (add_swav_loss: SwAV, swapped prediction of Sinkhorn-Knopp codes on --swav_num_prototypes "
                                        'prototypes; no target network; loss width 64, 128 or 256; always l2-normalised, --hidden_norm and '
                                        '--temperature are ignored) '
                                        "or 'vicreg' (add_vicreg_loss: VICReg, invariance + variance hinge + covariance, no negatives; loss "
                                        'width as for barlow, the official expander is 8192 wide; --hidden_norm and --temperature are ignored).  '
                                        'Ignored by --train_mode=finetune.'),
    ('gcl_dist', 'logsumexp', str, "MI355X build: distribution-matching term of the generalized loss: 'logsumexp' (decoupled NT-Xent), 'normal' or "
                                   "'uniform' (sliced Wasserstein distance to that prior; global batch <= 4096)."),
    ('gcl_lambda', 1.0, float, 'MI355X build: weight of the distribution-matching term (lambda_weight).'),
    ('gcl_loss_scaling', 1.0, float, 'MI355X build: factor on the whole generalized loss (loss_scaling).'),
    ('gcl_seed', 0, int, 'MI355X build: seed of the SWD projection basis and prior samples; the draws of a step depend on (gcl_seed, step) only.'),
    # the two corrections of NT-Xent itself (add_hard_negative_contrastive_loss), read under --contrastive_loss=ntxent only
    ('hard_negative_beta', 0.0, float, 'MI355X build: hard-negative re-weighting of NT-Xent (Robinson et al. 2021): every negative weighs '
                                       'exp(beta * s / temperature), differentiated through.  >= 0 and finite; 0 = NT-Xent.  A nonzero value '
                                       'needs --contrastive_loss=ntxent, --hidden_norm=true, a loss width of 64, 128 or 256 and '
                                       '--train_batch_size >= 2.  Ignored by --train_mode=finetune and --mode=eval.'),
    ('debiased_tau_plus', 0.0, float, 'MI355X build: debiasing correction of NT-Xent (Chuang et al. 2020): the class prior of a false negative, '
                                      'whose expected mass is taken out of the negative term (floored at M exp(-1 / temperature)).  In [0, 1); '
                                      '0 = NT-Xent.  Same requirements as --hard_negative_beta.'),
    # NNCLR: nearest-neighbour positives for NT-Xent (add_nn_contrastive_loss), read under --contrastive_loss=ntxent only
    ('nn_queue_size', 0, int, 'MI355X build: rows K of the support queue of NNCLR (after Dwibedi et al. 2021): the anchor of every row is '
                              'its nearest neighbour among the last K view-a embeddings of the global batch.  0 = NT-Xent.  A nonzero value '
                              'must be a multiple of --train_batch_size, at least that, and needs --contrastive_loss=ntxent, '
                              '--hidden_norm=true, a loss width of 64, 128 or 256, --train_batch_size >= 2 and both --hard_negative_beta and '
                              '--debiased_tau_plus at 0.  Ignored by --train_mode=finetune and --mode=eval.'),
    ('nn_queue_seed', 0, int, 'MI355X build: seed of the random unit rows the support queue of NNCLR starts from.'),
    # Barlow Twins (Zbontar et al. 2021) in place of NT-Xent for pretraining
    ('bt_lambda', 0.0051, float, 'MI355X build: weight of the off-diagonal (redundancy-reduction) term of the Barlow Twins loss (lambda_weight).'),
    ('bt_loss_scaling', 1.0, float, 'MI355X build: factor on the whole Barlow Twins loss (loss_scaling).'),
    # VICReg (Bardes, Ponce, LeCun 2022) in place of NT-Xent for pretraining
    ('vicreg_sim_coeff', 25.0, float, 'MI355X build: weight of the invariance term of the VICReg loss (sim_coeff).  >= 0.'),
    ('vicreg_std_coeff', 25.0, float, 'MI355X build: weight of the variance (hinge on the standard deviation) term of the VICReg loss (std_coeff).  >= 0.'),
    ('vicreg_cov_coeff', 1.0, float, 'MI355X build: weight of the covariance term of the VICReg loss (cov_coeff).  >= 0.'),
    # BYOL (Grill et al. 2020) in place of NT-Xent for pretraining: a momentum target network and a predictor on the online side
    ('byol_tau_base', 0.996, float, 'MI355X build: base decay of the target network\'s moving average; step k of K uses '
                                    'tau_k = 1 - (1 - byol_tau_base) * (cos(pi k / K) + 1) / 2.  In [0, 1].'),
    ('byol_pred_hidden_dim', 4096, int, 'MI355X build: hidden width of the BYOL predictor (dense + BN + ReLU, dense): a multiple of 64 in [64, 8192].'),
    # MoCo v2 (He et al. 2020; Chen et al. 2020) in place of NT-Xent for pretraining: a momentum target network and a queue of its keys
    ('moco_queue_size', 65536, int, 'MI355X build: rows K of the MoCo key queue: a multiple of 2 x train_batch_size, at least that and at most 1048576.'),
    ('moco_momentum', 0.999, float, 'MI355X build: constant decay m of the MoCo target network\'s moving average, t <- t + (1 - m) (o - t).  In [0, 1].'),
    ('moco_queue_seed', 0, int, 'MI355X build: seed of the random unit rows the MoCo queue starts from (the same on every replica).'),
    # DINO (Caron et al. 2021) in place of NT-Xent for pretraining: a momentum target network, a trained prototype layer and a centre
    ('dino_out_dim', 65536, int, 'MI355X build: number K of DINO prototypes (the width of the two softmaxes): 2 .. 1048576.'),
    ('dino_student_temp', 0.1, float, 'MI355X build: temperature of the DINO student softmax.  > 0.'),
    ('dino_teacher_temp', 0.04, float, 'MI355X build: final temperature of the DINO teacher softmax.  > 0.'),
    ('dino_warmup_teacher_temp', 0.04, float, 'MI355X build: teacher temperature at step 0; it moves linearly to --dino_teacher_temp over '
                                              '--dino_warmup_teacher_temp_epochs.  > 0.'),
    ('dino_warmup_teacher_temp_epochs', 0, int, 'MI355X build: epochs of the teacher temperature warm-up.  >= 0.'),
    ('dino_center_momentum', 0.9, float, 'MI355X build: decay m of the DINO centre, c <- m c + (1 - m) (batch mean of the teacher logits).  In [0, 1].'),
    ('dino_momentum', 0.996, float, 'MI355X build: base decay of the DINO target network; it follows the cosine schedule of BYOL to 1.  In [0, 1].'),
    ('dino_freeze_last_layer_epochs', 1, int, 'MI355X build: epochs during which the DINO prototypes take no update at all.  >= 0.'),
    # SwAV (Caron et al. 2020) in place of NT-Xent for pretraining: a trained prototype layer and Sinkhorn-Knopp codes, no target network
    ('swav_num_prototypes', 3000, int, 'MI355X build: number K of SwAV prototypes: 2 .. 1048576.'),
    ('swav_epsilon', 0.05, float, 'MI355X build: entropy regularisation of the SwAV Sinkhorn-Knopp assignment (the temperature of the codes).  > 0.'),
    ('swav_temperature', 0.1, float, 'MI355X build: temperature of the SwAV student softmax.  > 0.'),
    ('swav_sinkhorn_iterations', 3, int, 'MI355X build: Sinkhorn-Knopp iterations of the SwAV codes: 1 .. 16.'),
    ('swav_freeze_prototypes_epochs', 1, int, 'MI355X build: epochs during which the SwAV prototypes take no update at all.  >= 0.'),
    # SwAV multi-crop (Caron et al. 2020, section 4): L low-resolution views through a second encoder pass, against both global codes
    ('swav_local_crops', 0, int, 'MI355X build: number L of local (low-resolution) views of SwAV multi-crop: 0 (off) .. 8.'),
    ('swav_local_crop_size', 96, int, 'MI355X build: side of the local views in pixels: at most image_size, a multiple of the stem stride.'),
    ('swav_local_crop_min_scale', 0.05, float, 'MI355X build: smallest area share of a local crop; also its min_object_covered.'),
    ('swav_local_crop_max_scale', 0.14, float, 'MI355X build: largest area share of a local crop: 0 < min < max <= 1.'),
    # DINO multi-crop (Caron et al. 2021): L low-resolution student views through a second encoder pass, against both global teacher views
    ('dino_local_crops', 0, int, 'MI355X build: number L of local (low-resolution) views of DINO multi-crop: 0 (off) .. 8.'),
    ('dino_local_crop_size', 96, int, 'MI355X build: side of the DINO local views in pixels: at most image_size, a multiple of the stem stride.'),
    ('dino_local_crop_min_scale', 0.05, float, 'MI355X build: smallest area share of a DINO local crop; also its min_object_covered.'),
    ('dino_local_crop_max_scale', 0.14, float, 'MI355X build: largest area share of a DINO local crop: 0 < min < max <= 1.'),
    # DropBlock in the bottleneck blocks (tf2/resnet.py:81-157; the reference has the arguments of resnet() and no flag for them)
    ('dropblock_keep_probs', '', str, "MI355X build: DropBlock keep probabilities of block groups 1..4, four comma-separated values; 'none' or '1' "
                                      "switches a group off (e.g. none,none,0.9,0.9).  Default empty: no DropBlock."),
    ('dropblock_size', None, int, 'MI355X build: DropBlock block size; required when any keep probability is active.'),
    ('dropblock_seed', 0, int, 'MI355X build: seed of the DropBlock noise; the draws of a site depend on (dropblock_seed, step, replica, site) only.'),
    # weighted k-NN evaluation of the frozen encoder (Wu et al. 2018; simclr_amd/knn.py): no trained head
    ('knn_eval', False, bool, 'MI355X build: --mode=eval / train_then_eval also classify --eval_split by a weighted k-NN vote over the encoder '
                              'features of --train_split (evaluation preprocessing) and write knn_result.json; runs with or without a linear head.'),
    ('knn_k', 200, int, 'MI355X build: neighbours per query of the k-NN evaluation (1..256).'),
    ('knn_temperature', 0.07, float, 'MI355X build: temperature of the k-NN vote weights exp(similarity / temperature).'),
    ('knn_bank_examples', 0, int, 'MI355X build: examples of --train_split in the k-NN bank: 0 = the whole split, n > 0 = the first n positions of '
                                  'epoch_permutation(data_seed, 0, N).  --dataset=synthetic: a bank of random images, at most 8 eval batches.'),
    # cached-feature linear probe (simclr_amd/logreg.py): l2-regularised softmax regression on frozen features, fitted with L-BFGS
    ('logreg_eval', False, bool, 'MI355X build: --mode=eval / train_then_eval also encode --train_split once under evaluation preprocessing, fit an '
                                 'l2-regularised multinomial logistic regression on the standardised features with L-BFGS, score '
                                 '--eval_split with it and write logreg_result.json; runs with or without a linear head.'),
    ('logreg_l2', '1e-4', str, 'MI355X build: l2 coefficient of the probe (weights and bias), one value > 0 or a comma list: the values are '
                               'fitted in the order given, each warm-started from the one before, all are reported, none is selected.'),
    ('logreg_max_iterations', 200, int, 'MI355X build: L-BFGS iteration cap of the probe (1..10000).'),
    ('logreg_tolerance', 1e-5, float, 'MI355X build: the probe stops when |g|_inf <= logreg_tolerance * max(1, |f|); in (0, 1).'),
    ('logreg_history', 10, int, 'MI355X build: (s, y) pairs the L-BFGS recursion of the probe keeps (1..64).'),
    ('logreg_bank_examples', 0, int, 'MI355X build: examples of --train_split the probe is fitted on: 0 = the whole split, n > 0 = the first n '
                                     'positions of epoch_permutation(data_seed, 0, N) (the rule of --knn_bank_examples).'),
    # k-means clustering evaluation (simclr_amd/kmeans.py): spherical k-means on frozen features, scored against the labels
    ('kmeans_eval', False, bool, 'MI355X build: --mode=eval / train_then_eval also cluster the l2-normalised encoder features of --train_split '
                                 '(evaluation preprocessing) with spherical k-means, score --eval_split by NMI, ARI and cluster accuracy '
                                 'and write kmeans_result.json; runs with or without a linear head.'),
    ('kmeans_k', 0, int, 'MI355X build: clusters of the k-means evaluation (2..16384); 0 = the class count of the dataset.'),
    ('kmeans_restarts', 1, int, 'MI355X build: k-means restarts (1..16); the one with the lowest objective on the bank is scored.'),
    ('kmeans_max_iterations', 50, int, 'MI355X build: Lloyd iteration cap of a restart (1..1000).'),
    ('kmeans_tolerance', 1e-6, float, 'MI355X build: a restart stops when J_prev - J <= kmeans_tolerance * J_prev (or no assignment '
                                      'changed); in [0, 1).'),
    ('kmeans_seed', 0, int, 'MI355X build: restart r starts from rows drawn with numpy.random.default_rng([kmeans_seed, r]).'),
    ('kmeans_bank_examples', 0, int, 'MI355X build: examples of --train_split that are clustered: 0 = the whole split, n > 0 = the first n '
                                     'positions of epoch_permutation(data_seed, 0, N) (the rule of --knn_bank_examples).'),
    # eigen-spectrum evaluation (simclr_amd/spectrum.py): the covariance spectrum of the unnormalised encoder output, label-free
    ('spectrum_eval', False, bool, 'MI355X build: --mode=eval / train_then_eval also compute the eigenvalues of the covariance of the '
                                   'encoder features of --train_split (evaluation preprocessing, not normalised), score them (RankMe, '
                                   'participation ratio, numerical rank, power-law decay) and write spectrum_result.json; needs no labels.'),
    ('spectrum_bank_examples', 0, int, 'MI355X build: examples of --train_split whose covariance is taken: 0 = the whole split, n > 0 = the '
                                       'first n positions of epoch_permutation(data_seed, 0, N) (the rule of --knn_bank_examples).'),
    ('spectrum_rank_threshold', 1e-6, float, 'MI355X build: the numerical rank counts the eigenvalues above spectrum_rank_threshold times '
                                             'the largest; in (0, 1).'),
    ('spectrum_alpha_first', 10, int, 'MI355X build: first eigenvalue index (1-based) of the power-law fit of eval/spectrum_alpha; >= 1.'),
    ('spectrum_alpha_last', 0, int, 'MI355X build: last eigenvalue index of the power-law fit; 0 = the numerical rank, else >= '
                                    'spectrum_alpha_first + 7.'),
    # asymmetric view augmentation (flags.aug_plan): per-view blur and solarization of the two global views, jitter components.
    # None = take the column from --aug_recipe.  Read in pretraining only: --train_mode=finetune and --mode=eval ignore all five.
    ('aug_recipe', 'simclr', str, "MI355X build: augmentation recipe of the two global views, 'simclr' (default: blur 0.5 / 0.5, no "
                                  "solarization, jitter components 0.8,0.8,0.8,0.2), 'byol' (the asymmetric recipe this project defines "
                                  'for BYOL, Barlow Twins, VICReg and the global views of DINO: view a always blurred and never solarized, '
                                  "view b blurred with probability 0.1 and solarized with probability 0.2, components 0.4,0.4,0.2,0.1) or "
                                  "'mocov2' (blur 0.5 / 0.5, no solarization, components 0.4,0.4,0.4,0.1).  Independent of "
                                  '--contrastive_loss: nothing is switched on implicitly.  Local views of multi-crop keep blur 0.5 and no '
                                  'solarization; they take the jitter components.'),
    ('blur_probs', None, str, "MI355X build: 'pa,pb', blur probability of global view a (channels 0:3) and b; overrides the recipe's.  "
                              'Each in [0, 1].  --use_blur=False zeroes both and leaves solarization on.'),
    ('solarize_probs', None, str, "MI355X build: 'pa,pb', probability that global view a / b is solarized after the blur's clip; "
                                  "overrides the recipe's.  Each in [0, 1]."),
    ('solarize_threshold', 0.5, float, 'MI355X build: an element v >= threshold of a solarized image becomes 1 - v (an element equal to '
                                       'the threshold inverts).  In [0, 1].'),
    ('color_jitter_components', None, str, "MI355X build: 'b,c,s,h', the brightness, contrast, saturation and hue ranges per unit of "
                                           "--color_jitter_strength; overrides the recipe's.  Each >= 0, hue <= 0.5."),
    # label-free representation diagnostics (metrics.representation_stats, csrc/repr.hip): the same four numbers under every loss
    ('repr_metrics_steps', 0, int, 'MI355X build: every K-th pretraining step (those with (step + 1) % K == 0) measures alignment, '
                                   'uniformity, the per-feature standard deviation and the participation ratio of the l2-normalised online '
                                   'projection over the global batch and logs train/repr_align, train/repr_uniform, train/repr_std and '
                                   'train/repr_rank.  0 = off (default).  K > 0 needs a loss width that is a multiple of 64 in [64, 8192] and '
                                   '2 <= --train_batch_size <= 65536.  Read-only: the weights are bitwise those of K = 0.  Ignored by '
                                   '--train_mode=finetune and --mode=eval.'),
    ('repr_uniform_t', 2.0, float, 'MI355X build: scale t of the uniformity log mean exp(-t |z_a - z_b|^2).  In (0, 16].'),
]


LOCAL_CROP_LOSSES = ('swav', 'dino')      # the losses multi-crop is built for: each has its own four flags, <loss>_local_crop*


def local_crop_flags(flags=None):
    """(L, size, min_scale, max_scale) of the multi-crop flags of --contrastive_loss ('swav' or 'dino'), L = 0 for every other loss.
    The flags only: run.local_crop_plan adds that fine-tuning and evaluation ignore them."""
    flags = FLAGS if flags is None else flags
    loss = getattr(flags, 'contrastive_loss', 'ntxent')
    if loss not in LOCAL_CROP_LOSSES:
        return 0, int(flags.swav_local_crop_size), float(flags.swav_local_crop_min_scale), float(flags.swav_local_crop_max_scale)
    get = lambda name: getattr(flags, '%s_local_%s' % (loss, name))
    return int(get('crops')), int(get('crop_size')), float(get('crop_min_scale')), float(get('crop_max_scale'))


# --aug_recipe -> (blur probability of view a and b, solarize probability of view a and b, jitter components b, c, s, h).  'byol' is
# the asymmetric recipe of BYOL, Barlow Twins, VICReg and DINO's global views as this project defines it (a choice, not a parity claim)
AUG_RECIPES = {
    'simclr': ((0.5, 0.5), (0.0, 0.0), (0.8, 0.8, 0.8, 0.2)),
    'byol': ((1.0, 0.1), (0.0, 0.2), (0.4, 0.4, 0.2, 0.1)),
    'mocov2': ((0.5, 0.5), (0.0, 0.0), (0.4, 0.4, 0.4, 0.1)),
}
AugPlan = collections.namedtuple('AugPlan', 'recipe use_blur blur_probs solarize_probs solarize_threshold jitter_components')


def _number_list(flag, text, n):
    """'a,b,...' (or a sequence) -> n floats; ValueError naming the flag for another length or a non-number."""
    parts = list(text) if isinstance(text, (list, tuple)) else [t.strip() for t in str(text).split(',')]
    if len(parts) != n:
        raise ValueError('--%s needs %d comma-separated numbers (got %r)' % (flag, n, text))
    try:
        return tuple(float(t) for t in parts)
    except (TypeError, ValueError):
        raise ValueError('--%s: %r is not a list of numbers' % (flag, text))


def aug_plan(flags=None):
    """The resolved augmentation plan of the two global views -- the ONE reader of --aug_recipe, --blur_probs, --solarize_probs,
    --solarize_threshold and --color_jitter_components (the model, run.py and data.py call it): the recipe's row with every
    explicitly given flag in place of its column.  --use_blur=False zeroes the blur probabilities and leaves solarization on;
    --color_jitter_strength keeps scaling the components (data_util.draw_train_params).  Outside pretraining
    (--train_mode=finetune, --mode=eval) the five flags are not read: the plan is the `simclr` one.
    ValueError naming the flag -- run.main raises it before any device work -- for an unknown recipe, a list of the wrong length
    or with a non-number, a probability or the threshold outside [0, 1] or NaN, a negative or NaN component, a hue component
    above 0.5."""
    flags = FLAGS if flags is None else flags
    use_blur = bool(getattr(flags, 'use_blur', True))
    pretrain = getattr(flags, 'train_mode', 'pretrain') == 'pretrain' and getattr(flags, 'mode', 'train') != 'eval'
    recipe = getattr(flags, 'aug_recipe', 'simclr') if pretrain else 'simclr'
    if recipe not in AUG_RECIPES:
        raise ValueError("--aug_recipe must be 'simclr', 'byol' or 'mocov2' (got %r)" % (recipe,))
    blur, sol, comp = AUG_RECIPES[recipe]
    thr = 0.5
    if pretrain:
        given = lambda name: getattr(flags, name, None) not in (None, '')
        if given('blur_probs'):
            blur = _number_list('blur_probs', flags.blur_probs, 2)
        if given('solarize_probs'):
            sol = _number_list('solarize_probs', flags.solarize_probs, 2)
        if given('color_jitter_components'):
            comp = _number_list('color_jitter_components', flags.color_jitter_components, 4)
        try:
            thr = float(getattr(flags, 'solarize_threshold', 0.5))
        except (TypeError, ValueError):
            raise ValueError('--solarize_threshold: %r is not a number' % (flags.solarize_threshold,))
    for name, probs in (('blur_probs', blur), ('solarize_probs', sol)):
        if not all(0.0 <= p <= 1.0 for p in probs):                       # (NaN fails the comparison)
            raise ValueError('--%s: a probability lies in [0, 1] (got %r)' % (name, probs))
    if not 0.0 <= thr <= 1.0:
        raise ValueError('--solarize_threshold must lie in [0, 1] (got %r)' % (thr,))
    if not all(c >= 0.0 for c in comp):
        raise ValueError('--color_jitter_components: a component is a number >= 0 (got %r)' % (comp,))
    if comp[3] > 0.5:
        raise ValueError('--color_jitter_components: the hue component is at most 0.5 (got %r)' % (comp[3],))
    if not use_blur:
        blur = (0.0, 0.0)
    return AugPlan(recipe, use_blur, tuple(blur), tuple(sol), thr, tuple(comp))


def parse_dropblock_keep_probs(text):
    """--dropblock_keep_probs -> the `dropblock_keep_probs` argument of resnet(): None for the empty default, else a list of four
    entries, None ('none' / '1': off) or a float in (0, 1).  ValueError for anything else."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    if isinstance(text, (list, tuple)):
        parts = list(text)
    else:
        parts = [t.strip() for t in str(text).split(',')]
    if len(parts) != 4:
        raise ValueError('--dropblock_keep_probs needs four comma-separated values, one per block group (got %r)' % (text,))
    out = []
    for t in parts:
        if t is None or (isinstance(t, str) and t.lower() == 'none'):
            out.append(None)
            continue
        try:
            v = float(t)
        except ValueError:
            raise ValueError("--dropblock_keep_probs: %r is neither a number nor 'none'" % (t,))
        if not 0.0 < v <= 1.0:
            raise ValueError('--dropblock_keep_probs: a keep probability lies in (0, 1] (got %r)' % (t,))
        out.append(None if v == 1.0 else v)
    return out


def check_dropblock_flags(flags=None):
    """The `dropblock_keep_probs` / `dropblock_size` arguments of resnet() from the flags; raises ValueError -- before any device
    work -- for a malformed list, or an active keep probability without a positive --dropblock_size."""
    flags = FLAGS if flags is None else flags
    probs = parse_dropblock_keep_probs(getattr(flags, 'dropblock_keep_probs', ''))
    size = getattr(flags, 'dropblock_size', None)
    if probs is not None and any(p is not None for p in probs):
        if size is None or int(size) < 1:
            raise ValueError('--dropblock_keep_probs=%s needs a positive --dropblock_size (got %r)' % (flags.dropblock_keep_probs, size))
    return probs, size


class _Flags:
    def __init__(self):
        self.reset()

    def reset(self):
        for name, default, _, _ in _DEFS:
            setattr(self, name, default)

    def set_default(self, name, value):
        """Change the DEFAULT of a flag for this process (what reset() restores) -- test harnesses that calibrate on a specific mode."""
        for i, (n, _, typ, hlp) in enumerate(_DEFS):
            if n == name:
                _DEFS[i] = (n, value, typ, hlp)
                setattr(self, name, value)
                return
        raise AttributeError('Unknown flag %r' % name)

    def flag_values_dict(self):
        return {name: getattr(self, name) for name, _, _, _ in _DEFS}

    def update(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('Unknown flag %r' % k)
            setattr(self, k, v)
        return self

    @contextlib.contextmanager
    def override(self, **kw):
        """Flag values for the duration of a `with` block: a second model of another configuration (the distillation teacher) is
        built and called under it, while everything else keeps reading the process's flags."""
        old = {k: getattr(self, k) for k in kw}
        self.update(**kw)
        try:
            yield self
        finally:
            for k, v in old.items():
                setattr(self, k, v)

    def parse(self, argv):
        """absl-style parsing: --name=value, --name value, --flag / --noflag for booleans."""
        p = argparse.ArgumentParser(allow_abbrev=False)
        for name, default, typ, hlp in _DEFS:
            if typ is bool:
                p.add_argument('--' + name, nargs='?', const=True, default=default,
                               type=lambda s: str(s).lower() in ('1', 'true', 't', 'yes', 'y'), help=hlp)
                p.add_argument('--no' + name, dest=name, action='store_false', help=argparse.SUPPRESS)
            else:
                p.add_argument('--' + name, default=default, type=typ, help=hlp)
        ns = p.parse_args(argv)
        for name, _, _, _ in _DEFS:
            setattr(self, name, getattr(ns, name))
        return self


FLAGS = _Flags()

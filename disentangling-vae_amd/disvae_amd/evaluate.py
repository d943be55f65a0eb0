"""Evaluation with the API of disvae/evaluate.py on the native model.

* Test losses (``Evaluator.compute_losses``, evaluate.py:60-117): eval-mode forward (z = mean, vae.py:69-71) + the loss
  plugins with ``is_train=False`` (storer always kept, annealing = 1, losses.py:109,146-147), one stream of HIP launches
  per batch and ONE device->host copy for all logged scalars.
  Reference quirk: ``compute_losses`` returns from inside its batch loop (evaluate.py:116-117), i.e. it
  evaluates only the FIRST batch and divides by the number of batches.  Here every batch is evaluated and the mean is
  returned; ``reference_early_return=True`` reproduces the reference's numbers.
* MIG / AAM disentanglement metrics (``compute_metrics``, evaluate.py:119-317): q(z|x) of the whole data
  set through the native encoder, then the marginal and conditional entropy estimators -- N x D x 10 000 Gaussian
  log-densities + logsumexp per entropy, the kernel family of the beta-TCVAE estimator -- as ONE HIP launch sequence per
  entropy (``dvae_latent_entropy``) instead of 1 000 Python-driven [N, D, 10] torch chunks.  The few-element table
  arithmetic (mutual information, sort, MIG, AAM) stays on the host as in the reference.
* Importance-weighted log-likelihood (``compute_log_likelihood``, new): the mean over the data set of likelihood.log_likelihood
  (K samples per image, a private seeded generator), written to log_likelihood.log by ``__call__(is_log_likelihood=True)``.
* FactorVAE score (Kim & Mnih 2018, section 4) and beta-VAE score (Higgins et al. 2017, section 3), new
  (``compute_factor_scores`` / ``factor_scores_from_table``): rows of the table of posterior means drawn with one factor of
  variation fixed, the statistic of the 15 000 gathered groups (variance per dimension / mean absolute pair difference) and the
  majority vote as HIP launches on the table where it lies (libdvae_score_hip.so); only the [K, D] vote matrices, the variance
  vector and the beta-VAE classifier's [V, D] features cross to the host.  Definitions and defaults: disentanglement_lib's
  factor_vae.py / beta_vae.py.  Written to factor_scores.log by ``__call__(is_scores=True)``.
* Discretised MIG (Locatello et al. 2019), modularity (Ridgeway & Mozer 2018) and the continuous-factor SAP score (Kumar et al.
  2018), new (``compute_information_scores`` / ``information_scores_from_table``): the centred moments and the D x K joint
  histograms of the table of posterior means against the factors as two HIP passes on the table where it lies
  (libdvae_info_hip.so; the factor values are digits of the row number and never exist in memory); the moments and the integer
  counts cross to the host, where the scores are combined in fp64.  Definitions: disentanglement_lib's mig.py,
  modularity_explicitness.py and sap_score.py.  Written to information_scores.log by ``__call__(is_information=True)``.
* Interventional robustness score (Suter et al. 2019), new (``compute_irs`` / ``irs_from_table``): per (binned) factor value the
  mean of every latent and a quantile of the absolute deviations from it -- group means and an exact segmented radix select as HIP
  launches on the table where it lies (libdvae_irs_hip.so); the counts and two order statistics per (group, latent) cross to
  the host, where the quantiles are interpolated and the score is combined in fp64.  Definition: disentanglement_lib's irs.py.
  Written to irs.log by ``__call__(is_irs=True)``.
* Label-free scores (disentanglement_lib's unsupervised_metrics.py), new (``compute_unsupervised_scores`` /
  ``unsupervised_scores_from_table``): Gaussian total correlation, Gaussian Wasserstein correlation and the mean pairwise
  mutual information of the discretised latents, for data sets WITHOUT known factors (CelebA, Chairs, MNIST).  The D x D
  covariance in fp64 and the D (D - 1) / 2 pair histograms as two HIP passes on the table where it lies
  (libdvae_unsup_hip.so); the statistics cross to the host, where the scores are combined in fp64.
  Written to unsupervised_scores.log by ``__call__(is_unsupervised=True)``.
* Unsupervised disentanglement ranking (Duan et al. 2020; disentanglement_lib's udr.py), new (``compute_udr`` /
  ``udr_from_tables``): model selection WITHOUT labels -- a model of a sweep scores high when its informative latents match, one
  to one, those of the other models.  The KL divergence per dimension and the tie-averaged ranks of every column of every
  model's table as HIP launches (libdvae_udr_hip.so: a segmented radix sort), the correlation of the rank tables by
  dvae_unsup_moments; the [D, D] correlation blocks cross to the host, where the Lasso form is fitted and the scores are
  combined in fp64.  Written to udr.log by ``__call__(udr_models=[...])``.
* DCI -- disentanglement, completeness, informativeness (Eastwood & Williams 2018; disentanglement_lib's dci.py), new
  (``compute_dci`` / ``dci_from_table``): per factor of variation a gradient-boosted tree classifier (scikit-learn's
  GradientBoostingClassifier with default arguments, restated) is FITTED ON THE DEVICE on the posterior means where they lie
  (libdvae_dci_hip.so: every stage of every factor is enqueued without a read-back); the [D] importances and the accuracies cross
  to the host, where the entropies of the [D, K] importance matrix are combined in fp64.  Written to dci.log by
  ``__call__(is_dci=True)``.
* Prediction-based scores, new, on the entry points that are there (no new kernel): the downstream task (Locatello et al. 2019,
  section 5.4; ``compute_downstream_task`` / ``downstream_task_from_table``), unfairness (Locatello et al. 2019b;
  ``compute_fairness`` / ``fairness_from_table``) and explicitness (Ridgeway & Mozer 2018; ``compute_explicitness`` /
  ``explicitness_from_table``).  The first two fit and evaluate DCI's boosted trees (libdvae_dci_hip.so; ``_BoostedFactor``, which
  dci_from_table shares) -- on growing training sets, and on rows whose sensitive factor was intervened on, predicted by row
  number without a copy of the table; the third ranks the class probabilities of the beta-VAE score's logistic regression with
  dvae_udr_ranks: a ROC AUC is a rank sum.  Written to downstream_task.log / fairness.log / explicitness.log by
  ``__call__(is_downstream=True, is_fairness=True, is_explicitness=True)``.
* Separability and informativeness per latent, label-free (Do & Tran 2020: SEPIN, WSEPIN and their relatives), new
  (``compute_separability_scores`` / ``separability_scores_from_entropies``): the per-dimension refinement of the total
  correlation.  On the samples of the ELBO decomposition, the leave-one-out joint entropies H[z_!=i] of every latent and the joint
  entropy from ONE pass over the S x N x D terms (libdvae_sep_hip.so), the marginal entropies by dvae_latent_entropy and the
  conditional entropies per dimension; 3 D + 1 entropies cross to the host, where the scores are combined in fp64.
  Written to separability_scores.log by ``__call__(is_separability=True)``.
* Interpretability, the factor-based half of Do & Tran 2020: RMIG and JEMMIG, with MIG-sup (Li et al. 2020) and DCIMIG
  (Sepliarskaia et al. 2019) from the same mutual-information matrix, new (``compute_interpretability_scores`` /
  ``interpretability_scores_from_table`` / ``interpretability_scores_from_mass``).  Unlike the MIG variants above these use the
  posterior VARIANCE: q(z_d | x) of every row is integrated over fixed bins (Gaussian tail differences in fp64) and summed per
  factor value in one HIP pass on the tables where they lie (libdvae_mass_hip.so; accumulators in LDS, fixed order); the
  [D, n_bins * sum(lat_sizes)] mass table crosses to the host, where the scores are combined in fp64.
  Written to interpretability_scores.log by ``__call__(is_interpretability=True)``.
* SAP with DISCRETE factors (Kumar et al. 2018; the branch of disentanglement_lib's sap_score.py that its shipped configuration
  selects, and so the SAP number of Locatello et al. 2019), new (``compute_sap_discrete`` / ``sap_discrete_from_table`` /
  ``sap_discrete_from_score_matrix``): entry [d, k] of the score matrix is the test accuracy of LinearSVC(C=0.01,
  class_weight="balanced") fitted on latent d alone.  With one feature every one-vs-rest squared-hinge problem has two unknowns,
  and Newton's method on the active set reaches its exact minimiser: all D x (classes of every factor) problems are fitted by ONE
  HIP launch on the table where it lies, their columns in LDS (libdvae_sap_hip.so), and two more launches count the correct
  predictions; the [D, K] counts, the coefficients and the iteration counts cross to the host.
  Written to sap_discrete.log by ``__call__(is_sap_discrete=True)``.
* BINNING-FREE MIG, modularity, MIG-sup and DCIMIG, and the InfoMEC scores InfoM and InfoC (Hsu et al. 2023), new
  (``compute_knn_information_scores`` / ``knn_information_scores_from_table`` / ``knn_information_scores_from_mi``): every
  mutual-information score above first puts the latent into bins; here I(z_d; v_k) is the k-nearest-neighbour estimate of Ross
  2014 between the continuous latent and the discrete factor (scikit-learn's _compute_mi_cd, without mutual_info_classif's
  rescaling and noise).  In one dimension that is a sort, a partition by label, a bounded neighbour walk and two binary searches
  per row, all integer-exact in the LDS of one workgroup (libdvae_knn_hip.so): two launches, and the neighbour counts' digamma
  sums [D, K, 4] and the class counts cross to the host, where the estimate is clipped at 0 and the scores are combined in fp64.
  Written to knn_information_scores.log by ``__call__(is_knn_information=True)``.
* LINEAR-SOFTMAX PROBES FITTED ON THE DEVICE and InfoE, the third score of the InfoMEC triple (Hsu et al. 2023), new
  (``fit_logistic_regression_device``; ``fit="device"`` of ``explicitness_from_table`` / ``factor_scores_from_table`` and their
  ``compute_*``; ``compute_infoe`` / ``infoe_from_table`` / ``infoe_from_log_loss``): the multinomial logistic regression of the
  beta-VAE score and of explicitness -- fit_logistic_regression's objective -- solved by a truncated Newton-CG iteration in fp64
  inside ONE HIP launch, a persistent workgroup per problem (libdvae_lr_hip.so), its probabilities, log-loss and counts of correct
  rows by a second launch; the coefficients, the solver's report and [K] sums cross to the host.  InfoE per factor is 1 - the
  probe's cross-entropy / that of the training rows' class frequencies.  The host fit stays the default of the two older scores.
  Written to infoe.log by ``__call__(is_infoe=True)``.
"""
import logging
import math
import numbers
import os
from collections import defaultdict
from timeit import default_timer

import numpy as np
import torch

from . import _dcilib, _evallib, _infolib, _irslib, _knnlib, _lib, _lrlib, _masslib, _saplib, _scorelib, _seplib, _udrlib, _unsuplib
from ._lib import call, ptr
from .engine import _stream
from .likelihood import _ScorePasses, check_rec_dist, log_likelihood
from .models.losses import FactorKLoss
from .utils.modelIO import save_metadata

TEST_LOSSES_FILE = "test_losses.log"
METRICS_FILENAME = "metrics.log"
METRIC_HELPERS_FILE = "metric_helpers.pth"
LOG_LIKELIHOOD_FILE = "log_likelihood.log"
ELBO_DECOMPOSITION_FILE = "elbo_decomposition.log"
FACTOR_SCORES_FILE = "factor_scores.log"
INFORMATION_SCORES_FILE = "information_scores.log"
IRS_FILE = "irs.log"
UNSUPERVISED_SCORES_FILE = "unsupervised_scores.log"
UDR_FILE = "udr.log"
DCI_FILE = "dci.log"
DOWNSTREAM_TASK_FILE = "downstream_task.log"
FAIRNESS_FILE = "fairness.log"
EXPLICITNESS_FILE = "explicitness.log"
SEPARABILITY_SCORES_FILE = "separability_scores.log"
INTERPRETABILITY_SCORES_FILE = "interpretability_scores.log"
SAP_DISCRETE_FILE = "sap_discrete.log"
KNN_INFORMATION_SCORES_FILE = "knn_information_scores.log"
INFOE_FILE = "infoe.log"


class Evaluator:
    def __init__(self, model, loss_f, device=torch.device("cpu"), logger=logging.getLogger(__name__),
                 save_dir="results", is_progress_bar=True, reference_early_return=False):
        self.device = device
        self.loss_f = loss_f
        self.model = model.to(self.device)
        self.logger = logger
        self.save_dir = save_dir
        self.is_progress_bar = is_progress_bar
        self.reference_early_return = reference_early_return
        self.logger.info("Testing Device: {}".format(self.device))

    def __call__(self, data_loader, is_metrics=False, is_losses=True, is_log_likelihood=False, n_samples=128,
                 is_decomposition=False, n_samples_decomposition=10000, is_scores=False, is_information=False,
                 is_irs=False, is_unsupervised=False, udr_models=None, is_dci=False, dci_args=None, is_downstream=False,
                 is_fairness=False, is_explicitness=False, downstream_args=None, fairness_args=None, explicitness_args=None,
                 is_separability=False, n_samples_separability=10000, is_interpretability=False, interpretability_args=None,
                 is_sap_discrete=False, sap_discrete_args=None, is_knn_information=False, knn_information_args=None,
                 is_infoe=False, infoe_args=None):
        """evaluate.py:60-95.  is_log_likelihood: also write compute_log_likelihood(data_loader, n_samples) to
        log_likelihood.log; is_decomposition: also write compute_elbo_decomposition(data_loader, n_samples_decomposition) to
        elbo_decomposition.log; is_scores: also write compute_factor_scores(data_loader) to factor_scores.log; is_information: also
        write compute_information_scores(data_loader), without its [D, K] matrices, to information_scores.log; is_irs: also write compute_irs(data_loader),
        its arrays as lists, to irs.log; is_unsupervised: also write compute_unsupervised_scores(data_loader), its arrays as lists and
        without its [D, D] matrix, to unsupervised_scores.log; udr_models (the other models of a sweep): also write
        compute_udr(data_loader, udr_models), its arrays as lists and without raw_correlations, to udr.log (the return value stays
        the reference's (metric, losses)); is_dci: also write compute_dci(data_loader, **dci_args), without its [D, K] matrix, to
        dci.log; is_downstream / is_fairness / is_explicitness: also write compute_downstream_task(data_loader, **downstream_args) to
        downstream_task.log, compute_fairness(data_loader, **fairness_args) to fairness.log and compute_explicitness(data_loader,
        **explicitness_args) to explicitness.log, their arrays as lists; is_separability: also write
        compute_separability_scores(data_loader, n_samples_separability) to separability_scores.log; is_interpretability: also
        write compute_interpretability_scores(data_loader, **interpretability_args), without its [D, K] matrices, to
        interpretability_scores.log; is_sap_discrete: also write compute_sap_discrete(data_loader, **sap_discrete_args), without
        its matrices and coefficients, to sap_discrete.log; is_knn_information: also write
        compute_knn_information_scores(data_loader, **knn_information_args), without its [D, K] matrices, to
        knn_information_scores.log; is_infoe: also write compute_infoe(data_loader, **infoe_args), its arrays as lists and without
        the solver's [K, 4] report, to infoe.log."""
        start = default_timer()
        is_still_training = self.model.training
        self.model.eval()
        matrices, nothing = (lambda k, v: isinstance(v, np.ndarray) and v.ndim > 1), (lambda k, v: False)
        # (wanted, what is being computed, the call, what the log and the file leave out (None: the result as it is; else the
        # arrays that stay become lists), the label of the result line, the file)
        outputs = [
            (is_metrics, 'metrics', lambda: self.compute_metrics(data_loader), None, 'Losses', METRICS_FILENAME),
            (is_losses, 'losses', lambda: self.compute_losses(data_loader), None, 'Losses', TEST_LOSSES_FILE),
            (is_log_likelihood, 'the importance-weighted log-likelihood',
             lambda: self.compute_log_likelihood(data_loader, n_samples=n_samples), None, 'Log-likelihood', LOG_LIKELIHOOD_FILE),
            (is_decomposition, 'the ELBO decomposition over the data set',
             lambda: self.compute_elbo_decomposition(data_loader, n_samples=n_samples_decomposition), None, 'ELBO decomposition',
             ELBO_DECOMPOSITION_FILE),
            (is_scores, 'the FactorVAE and beta-VAE scores', lambda: self.compute_factor_scores(data_loader), None,
             'Disentanglement scores', FACTOR_SCORES_FILE),
            (is_information, 'the discretised MIG, modularity and SAP scores', lambda: self.compute_information_scores(data_loader),
             matrices, 'Information scores', INFORMATION_SCORES_FILE),
            (is_irs, 'the interventional robustness score', lambda: self.compute_irs(data_loader), nothing, 'IRS', IRS_FILE),
            (is_unsupervised, 'the label-free scores', lambda: self.compute_unsupervised_scores(data_loader), matrices,
             'Unsupervised scores', UNSUPERVISED_SCORES_FILE),
            (udr_models is not None, 'the unsupervised disentanglement ranking', lambda: self.compute_udr(data_loader, udr_models),
             lambda k, v: k == "raw_correlations", 'UDR', UDR_FILE),
            (is_dci, 'the DCI scores', lambda: self.compute_dci(data_loader, **(dci_args or {})),
             lambda k, v: isinstance(v, np.ndarray), 'DCI', DCI_FILE),
            (is_downstream, 'the downstream-task accuracies', lambda: self.compute_downstream_task(data_loader, **(downstream_args or {})),
             None, 'Downstream task', DOWNSTREAM_TASK_FILE),
            (is_fairness, 'the unfairness scores', lambda: self.compute_fairness(data_loader, **(fairness_args or {})), nothing,
             'Fairness', FAIRNESS_FILE),
            (is_explicitness, 'the explicitness score', lambda: self.compute_explicitness(data_loader, **(explicitness_args or {})),
             nothing, 'Explicitness', EXPLICITNESS_FILE),
            (is_separability, 'the separability scores',
             lambda: self.compute_separability_scores(data_loader, n_samples=n_samples_separability), None, 'Separability scores',
             SEPARABILITY_SCORES_FILE),
            (is_interpretability, 'the RMIG, JEMMIG, MIG-sup and DCIMIG scores',
             lambda: self.compute_interpretability_scores(data_loader, **(interpretability_args or {})), matrices,
             'Interpretability scores', INTERPRETABILITY_SCORES_FILE),
            (is_sap_discrete, 'the discrete-factor SAP score', lambda: self.compute_sap_discrete(data_loader, **(sap_discrete_args or {})),
             matrices, 'SAP (discrete factors)', SAP_DISCRETE_FILE),
            (is_knn_information, 'the binning-free MIG, InfoM and InfoC scores',
             lambda: self.compute_knn_information_scores(data_loader, **(knn_information_args or {})), matrices,
             'k-NN information scores', KNN_INFORMATION_SCORES_FILE),
            (is_infoe, 'the InfoE score', lambda: self.compute_infoe(data_loader, **(infoe_args or {})), matrices, 'InfoE', INFOE_FILE),
        ]
        written = {}
        for wanted, what, compute, left_out, label, filename in outputs:
            if not wanted:
                continue
            self.logger.info('Computing {}...'.format(what))
            result = compute()
            if left_out is not None:
                result = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in result.items() if not left_out(k, v)}
            self.logger.info('{}: {}'.format(label, result))
            os.makedirs(self.save_dir, exist_ok=True)
            save_metadata(result, self.save_dir, filename=filename)
            written[filename] = result
        if is_still_training:
            self.model.train()
        self.logger.info('Finished evaluating after {:.1f} min.'.format((default_timer() - start) / 60))
        return None, written.get(TEST_LOSSES_FILE)       # (metric, losses) of the reference; metric stays None, also with is_metrics

    def compute_losses(self, dataloader):
        """evaluate.py:97-117."""
        storer = defaultdict(list)
        n = len(dataloader)
        takes_labels = getattr(self.loss_f, "takes_labels", False)
        for data, labels in dataloader:
            data = data.to(self.device)
            if isinstance(self.loss_f, FactorKLoss):
                self.loss_f.call_optimize(data, self.model, None, storer)     # evaluate.py:112-114
            elif takes_labels:                                                # SemiSupervisedVaeLoss: the batch's row numbers, if any
                self.loss_f.fused_step(data, self.model, None, storer,
                                       labels=labels.to(self.device) if torch.is_tensor(labels) else None)
            else:
                self.loss_f.fused_step(data, self.model, None, storer)
            if self.reference_early_return:
                return {k: sum(v) / n for k, v in storer.items()}
        return {k: sum(v) / len(v) for k, v in storer.items()}

    def compute_log_likelihood(self, dataloader, n_samples=128, seed=0):
        """Mean over the data set of the importance-weighted estimate of log p(x) (nats per image; likelihood.log_likelihood)
        with n_samples samples of q(z|x) per image under the loss's rec_dist -- the bound itself for bernoulli, up to the
        likelihood's missing normalising constant for gaussian / laplace.  The draws come from a private generator seeded with
        `seed` (the same seed gives the same bits; the global random states are untouched); train / eval mode is restored."""
        rec_dist = getattr(self.loss_f, "rec_dist", "bernoulli")
        check_rec_dist(rec_dist)
        if int(n_samples) < 1:
            raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
        dev = _ScorePasses.of(self.model).check_device()
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        parts = [log_likelihood(self.model, data, n_samples=n_samples, rec_dist=rec_dist, generator=gen)
                 for data, _ in dataloader]
        per_image = torch.cat(parts).cpu().double()
        return {"log_likelihood": per_image.mean().item(), "n_samples": int(n_samples), "rec_dist": rec_dist}

    # ------------------------------------------------------------------ ELBO decomposition over the data set
    def compute_elbo_decomposition(self, dataloader, n_samples=10000, seed=0, sample_idx=None, eps=None):
        """Decomposition of the data-set average of KL[q(z|x_n) || p(z)] (Chen et al. 2018, section 3) into index-code mutual
        information, total correlation and dimension-wise KL, each against the aggregate posterior q(z) = 1/N sum_n q(z|x_n)
        of ALL N images of the loader, estimated on S = n_samples samples z_s = mu_n(s) + exp(logvar_n(s) / 2) eps_s of S
        distinct images n(s) (n_samples=None: S = N, every image once in data-set order -- the paper's full estimate):

            H_z    = -1/S sum_s log q(z_s)                  joint entropy       (dvae_eval_joint_logq)
            H_z_d  = [-1/S sum_s log q_d(z_sd) for d]       marginal entropies  (dvae_latent_entropy on the [D, S] image of z)
            H_zCx  = -1/S sum_s log q(z_s | x_n(s))         conditional entropy (dvae_eval_sample_terms)
            mi     = H_z - H_zCx
            tc     = sum_d H_z_d - H_z
            dw_kl  = -sum_d H_z_d - 1/S sum_s log p(z_s)
            kl     = mi + tc + dw_kl                        (= 1/S sum_s [log q(z_s | x_n(s)) - log p(z_s)])

        Unlike the minibatch mi_loss / tc_loss / dw_kl_loss of the training log these do not depend on a batch size or a loss.
        The draws (rows = randperm(N)[:S], eps ~ N(0, I)) come from a private generator seeded with `seed`: the same seed gives
        the same bits, the global random states are untouched; sample_idx ([S] rows, each in [0, N)) / eps ([S, D]) inject
        them.  Train / eval mode is restored.  The handful of scalars is combined on the host."""
        table, n, dim, S, rows, noise, z = self._posterior_samples(dataloader, n_samples, seed, sample_idx, eps)
        dev = table.mean.device

        E = _evallib.lib()
        out = torch.empty(3 * S + 3 + dim, dtype=torch.float32, device=dev)       # logqz, logqz_condx, logpz, H_z, 2 means, H_z_d
        logqz, logqz_condx, logpz = out[:S], out[S:2 * S], out[2 * S:3 * S]
        scal = out[3 * S:]
        ws = torch.empty(max(E.dvae_eval_joint_logq_ws_floats(n, dim, S), _lib.lib().dvae_latent_entropy_ws_floats(n, dim, S)),
                         dtype=torch.float32, device=dev)
        st = _stream()
        _evallib.call("dvae_eval_joint_logq", ptr(z), ptr(table.mean), ptr(table.logvar), n, dim, S, ptr(ws), ptr(logqz),
                      ptr(scal), st)
        _evallib.call("dvae_eval_sample_terms", ptr(z), ptr(noise), ptr(table.logvar), ptr(rows), n, dim, S, ptr(logqz_condx),
                      ptr(logpz), scal.data_ptr() + 4, st)
        # dvae_latent_entropy reads a [D, S] image whose row d must hold the S samples of z_d: the TRANSPOSED copy of the [S, D]
        # samples.  This deliberately differs from _entropies below, which hands over the gathered [S, D] block as it lies in
        # memory to reproduce the reference's MIG numbers (its .view is a reshape that mixes dimensions): here there is no
        # reference to match, a reshape would evaluate q_d at samples of other dimensions and tc would not be 0 at D = 1.
        z_ds = z.t().contiguous()
        call("dvae_latent_entropy", ptr(z_ds), ptr(table.mean), ptr(table.logvar), n, dim, S, ptr(ws), scal.data_ptr() + 12, st)
        host = [float(v) for v in scal.cpu().double()]                           # ONE device->host copy
        H_z, mean_logqz_condx, mean_logpz, H_z_d = host[0], host[1], host[2], host[3:]
        H_zCx = -mean_logqz_condx
        mi = H_z - H_zCx
        tc = math.fsum(H_z_d) - H_z
        dw_kl = -math.fsum(H_z_d) - mean_logpz
        return {"H_z": H_z, "H_z_d": H_z_d, "H_zCx": H_zCx, "mi": mi, "tc": tc, "dw_kl": dw_kl, "kl": mi + tc + dw_kl,
                "n_samples": S, "n_data": n}

    def _posterior_samples(self, dataloader, n_samples, seed, sample_idx, eps):
        """What compute_elbo_decomposition and compute_separability_scores do before their kernels: the sizes and every check
        (before any device work), the table of q(z|x) over the whole data set, and the draws -- rows = randperm(N)[:S] and
        eps ~ N(0, I) from a private generator seeded with `seed`, or the injected sample_idx / eps -- so that the same seed
        gives both methods the same samples.  -> (table, N, D, S, rows [S], noise [S, D], z [S, D])."""
        # every size is known and checked before any device work: a DataLoader tells the length of its data set, a plain
        # sequence of batches is counted
        ds = getattr(dataloader, "dataset", None)
        n = len(ds) if ds is not None else sum(len(x) for x, _ in dataloader)
        dim = int(self.model.latent_dim)
        if sample_idx is not None:
            sample_idx = torch.as_tensor(sample_idx).to(torch.int64).reshape(-1)
            n_samples = int(sample_idx.numel())
        S = n if n_samples is None else int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be >= 1 (or None for the whole data set), got %r" % (n_samples,))
        if S > n:
            raise ValueError("n_samples=%d exceeds the %d images of the data set (samples are drawn without replacement)" % (S, n))
        if eps is not None and tuple(eps.shape) != (S, dim):
            raise ValueError("eps must have shape (%d, %d), got %s" % (S, dim, tuple(eps.shape)))
        if sample_idx is not None and not (0 <= int(sample_idx.min()) and int(sample_idx.max()) < n):
            raise ValueError("sample_idx must hold rows in [0, %d)" % n)            # (the kernels do not check them)
        table = _LatentTable(*self._encode(dataloader))
        if table.n != n:
            raise ValueError("the loader yielded %d images, its data set has %d" % (table.n, n))
        dev = table.mean.device
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        if sample_idx is not None:
            rows = sample_idx.to(dev)
        elif n_samples is None:
            rows = torch.arange(n, device=dev)
        else:
            rows = torch.randperm(n, generator=gen, device=dev)[:S].contiguous()
        noise = torch.randn(S, dim, generator=gen, device=dev) if eps is None else eps.to(dev, torch.float32).contiguous()
        mean_s, logvar_s = table.select(rows)
        z = (mean_s + torch.exp(0.5 * logvar_s) * noise).contiguous()
        return table, n, dim, S, rows, noise, z

    # ------------------------------------------------------------------ SEPIN / WSEPIN separability
    def compute_separability_scores(self, dataloader, n_samples=10000, seed=0, sample_idx=None, eps=None):
        """Separability and informativeness of every latent WITHOUT labels (Do & Tran 2020): how much latent i tells about the
        image that the other latents do not tell already, sepin[i] = I(x; z_i | z_!=i), its informativeness-weighted sum WSEPIN
        and what goes with them (separability_scores_from_entropies below), from entropies under the aggregate posterior of ALL
        N images of the loader, estimated on the S samples compute_elbo_decomposition draws (same arguments, checks, draws and
        error texts: the same seed gives both the same samples):

            H_loo[i]    = -1/S sum_s log q_!=i(z_s)         leave-one-out joint entropies, and
            H_z         = -1/S sum_s log q(z_s)             the joint entropy from the same pass  (dvae_sep_loo_logq)
            H_z_d[i]    = -1/S sum_s log q_i(z_si)          marginal entropies      (dvae_latent_entropy on the [D, S] image of z)
            H_cond_d[i] = -1/S sum_s log q(z_si | x_n(s))   conditional entropies   (dvae_sep_cond_terms)

        Returns the scores plus H_z, H_z_d, H_loo, H_cond_d, tc, n_samples, n_data.  A latent_dim above the kernels' largest
        raises ValueError before the encode pass.  Train / eval mode is restored; the scores are combined on the host in fp64."""
        dim = int(self.model.latent_dim)
        if dim > _seplib.MAX_D:
            raise ValueError("%d latent dimensions: the separability kernels take at most %d" % (dim, _seplib.MAX_D))
        table, n, dim, S, rows, noise, z = self._posterior_samples(dataloader, n_samples, seed, sample_idx, eps)
        dev = table.mean.device
        P = _seplib.lib()
        out64 = torch.empty(2 * dim + 1, dtype=torch.float64, device=dev)         # H_loo [D], H_z, H_cond_d [D]
        buf = torch.empty((dim + 1) * S + dim, dtype=torch.float32, device=dev)   # logq [D + 1, S], H_z_d [D]
        logq, H_z_d = buf[:(dim + 1) * S], buf[(dim + 1) * S:]
        ws = torch.empty(max(P.dvae_sep_loo_logq_ws_floats(n, dim, S), _lib.lib().dvae_latent_entropy_ws_floats(n, dim, S)),
                         dtype=torch.float32, device=dev)
        st = _stream()
        _seplib.call("dvae_sep_loo_logq", ptr(z), ptr(table.mean), ptr(table.logvar), n, dim, S, ptr(ws), ptr(logq), ptr(out64), st)
        _seplib.call("dvae_sep_cond_terms", ptr(noise), ptr(table.logvar), ptr(rows), n, dim, S, out64.data_ptr() + 8 * (dim + 1), st)
        z_ds = z.t().contiguous()                            # the [D, S] image, as compute_elbo_decomposition hands it over
        call("dvae_latent_entropy", ptr(z_ds), ptr(table.mean), ptr(table.logvar), n, dim, S, ptr(ws), ptr(H_z_d), st)
        host = torch.cat([out64, H_z_d.double()]).cpu().tolist()                  # ONE device->host copy
        H_loo, H_z, H_cond_d, H_marg = host[:dim], host[dim], host[dim + 1:2 * dim + 1], host[2 * dim + 1:]
        scores = separability_scores_from_entropies(H_z, H_marg, H_loo, H_cond_d)
        scores.update(H_z=H_z, H_z_d=H_marg, H_loo=H_loo, H_cond_d=H_cond_d, n_samples=S, n_data=n)
        return scores

    # ------------------------------------------------------------------ FactorVAE / beta-VAE scores
    def compute_factor_scores(self, dataloader, n_train=10000, n_eval=5000, batch_size=64, n_variance=10000,
                              active_threshold=0.05, seed=0, draws=None, fit="host"):
        """FactorVAE score and beta-VAE score of the model (factor_scores_from_table below, on the posterior means of the whole
        data set through the native encoder).  Requirements of compute_metrics: ``dataloader.dataset`` exposes ``lat_sizes`` /
        ``lat_names``, the loader iterates the data set in factor order and the data set enumerates ``lat_sizes``.  Every size
        is checked before any device work; train / eval mode is restored.  Returns {"factor_vae_train", "factor_vae_eval",
        "beta_vae_train", "beta_vae_eval", "n_active", "n_train", "n_eval", "batch_size"}.  fit="device": the beta-VAE score's
        classifier is fitted by libdvae_lr_hip.so (factor_scores_from_table)."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_score_sizes(n, lat_sizes, n_train, n_eval, batch_size, n_variance)
        _check_fit(fit, n_train, None, [len(lat_sizes)])
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return factor_scores_from_table(mean, lat_sizes, n_train=n_train, n_eval=n_eval, batch_size=batch_size,
                                        n_variance=n_variance, active_threshold=active_threshold, seed=seed, draws=draws,
                                        **({} if fit == "host" else {"fit": fit}))      # the default hands on what it always did

    # ------------------------------------------------------------------ discretised MIG / modularity / SAP
    def compute_information_scores(self, dataloader, n_samples=None, n_bins=20, seed=0):
        """Discretised MIG, modularity and continuous-factor SAP of the model (information_scores_from_table below, on the
        posterior means of the whole data set through the native encoder).  The data-set requirements and errors of
        compute_factor_scores; every size is checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_information_sizes(n, lat_sizes, n_bins, n_samples)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return information_scores_from_table(mean, lat_sizes, n_bins=n_bins, n_samples=n_samples, seed=seed)

    # ------------------------------------------------------------------ SAP with discrete factors
    def compute_sap_discrete(self, dataloader, n_train=10000, n_test=5000, C=0.01, seed=0):
        """The discrete-factor SAP score of the model (sap_discrete_from_table below, on the posterior means of the whole data set
        through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and argument is
        checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_sap_arguments(n, None, lat_sizes, n_train, n_test, C, seed, None)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return sap_discrete_from_table(mean, lat_sizes, n_train=n_train, n_test=n_test, C=C, seed=seed)

    # ------------------------------------------------------------------ binning-free MIG / InfoM / InfoC
    def compute_knn_information_scores(self, dataloader, n_samples=10000, n_neighbors=3, seed=0):
        """Binning-free MIG, modularity, MIG-sup, DCIMIG, InfoM and InfoC of the model (knn_information_scores_from_table below,
        on the posterior means of the whole data set through the native encoder).  The data-set requirements and errors of
        compute_factor_scores; every size and argument is checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_knn_arguments(n, None, lat_sizes, n_samples, n_neighbors, seed, None)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return knn_information_scores_from_table(mean, lat_sizes, n_samples=n_samples, n_neighbors=n_neighbors, seed=seed)

    # ------------------------------------------------------------------ RMIG / JEMMIG / MIG-sup / DCIMIG
    def compute_interpretability_scores(self, dataloader, n_samples=None, n_bins=100, z_range=(-4., 4.), seed=0):
        """RMIG and JEMMIG (Do & Tran 2020), MIG-sup (Li et al. 2020) and DCIMIG (Sepliarskaia et al. 2019) of the model
        (interpretability_scores_from_table below, on the posterior means AND log-variances of the whole data set through the
        native encoder: a latent whose posterior is as wide as its bins does not score like a sharp one).  The data-set
        requirements and errors of compute_factor_scores; every size and argument is checked before any device work; train /
        eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_interpretability_arguments(n, lat_sizes, n_bins, z_range, n_samples)
        mean, logvar = self._encode(dataloader, n, lat_sizes)
        return interpretability_scores_from_table(mean, logvar, lat_sizes, n_bins=n_bins, z_range=z_range, n_samples=n_samples,
                                                  seed=seed)

    # ------------------------------------------------------------------ interventional robustness score
    def compute_irs(self, dataloader, diff_quantile=0.99, factor_bins=20, n_samples=None, seed=0):
        """Interventional robustness score of the model (irs_from_table below, on the posterior means of the whole data set
        through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and argument is
        checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_irs_arguments(n, lat_sizes, diff_quantile, factor_bins, n_samples)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return irs_from_table(mean, lat_sizes, diff_quantile=diff_quantile, factor_bins=factor_bins, n_samples=n_samples, seed=seed)

    # ------------------------------------------------------------------ label-free scores
    def compute_unsupervised_scores(self, dataloader, n_samples=None, n_bins=20, seed=0):
        """Gaussian total correlation, Gaussian Wasserstein correlation and mean pairwise mutual information of the model's
        representation (unsupervised_scores_from_table below, on the posterior means of the whole data set through the native
        encoder).  The data set needs NO known factors of variation; every argument that can be is checked before any device
        work; train / eval mode is restored."""
        ds = getattr(dataloader, "dataset", None)
        _check_unsupervised_arguments(len(ds) if hasattr(ds, "__len__") else None, None, n_bins, n_samples)
        mean, _logvar = self._encode(dataloader)
        return unsupervised_scores_from_table(mean, n_bins=n_bins, n_samples=n_samples, seed=seed)

    # ------------------------------------------------------------------ unsupervised disentanglement ranking
    def compute_udr(self, dataloader, other_models, **kw):
        """UDR of ``self.model`` (model 0) and ``other_models`` (udr_from_tables below, on the posterior means and log-variances
        of the whole data set; ``kw`` are its keyword arguments).  The loader is walked ONCE and every batch goes through every
        model's native encoder, so the rows of the tables line up even on a shuffling loader.  The data set needs no known factors
        of variation; every argument that can be is checked before any device work; the train / eval mode of every model is
        restored."""
        models = [self.model] + list(other_models)
        ds = getattr(dataloader, "dataset", None)
        _check_udr_arguments(len(models), len(ds) if hasattr(ds, "__len__") else None, None, **kw)
        was_training = [m.training for m in models]
        chunks = [[] for _ in models]
        try:
            for m in models:
                m.to(self.device).eval()
            with torch.no_grad():
                for x, _label in dataloader:
                    x = x.to(self.device)
                    for i, m in enumerate(models):
                        chunks[i].append(m.encoder(x))
        finally:
            for m, training in zip(models, was_training):
                if training:
                    m.train()
        means = [torch.cat([mu for mu, _ in c]) for c in chunks]
        logvars = [torch.cat([lv for _, lv in c]) for c in chunks]
        return udr_from_tables(means, logvars, **kw)

    # ------------------------------------------------------------------ DCI
    def compute_dci(self, dataloader, n_train=10000, n_test=5000, seed=0, n_stages=100):
        """Disentanglement, completeness and informativeness of the model (dci_from_table below, on the posterior means of the
        whole data set through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and
        argument is checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_dci_arguments(n, None, lat_sizes, n_train, n_test, seed, None, n_stages)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return dci_from_table(mean, lat_sizes, n_train=n_train, n_test=n_test, seed=seed, n_stages=n_stages)

    # ------------------------------------------------------------------ downstream task / fairness / explicitness
    def compute_downstream_task(self, dataloader, n_train=(10, 100, 1000, 10000), n_test=5000, seed=0, n_stages=100):
        """Downstream-task accuracies and sample efficiency of the model (downstream_task_from_table below, on the posterior means
        of the whole data set through the native encoder).  The data-set requirements and errors of compute_factor_scores; every
        size and argument is checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_downstream_arguments(n, None, lat_sizes, n_train, n_test, seed, None, n_stages)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return downstream_task_from_table(mean, lat_sizes, n_train=n_train, n_test=n_test, seed=seed, n_stages=n_stages)

    def compute_fairness(self, dataloader, n_train=10000, n_test_per_value=100, seed=0, n_stages=100):
        """Unfairness of the model's representation (fairness_from_table below, on the posterior means of the whole data set
        through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and argument is
        checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_fairness_arguments(n, None, lat_sizes, n_train, n_test_per_value, seed, n_stages)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return fairness_from_table(mean, lat_sizes, n_train=n_train, n_test_per_value=n_test_per_value, seed=seed, n_stages=n_stages)

    def compute_explicitness(self, dataloader, n_train=10000, n_test=5000, seed=0, fit="host"):
        """Explicitness of the model's representation (explicitness_from_table below, on the posterior means of the whole data set
        through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and argument is
        checked before any device work; train / eval mode is restored.  fit="device": the K logistic regressions are fitted by
        libdvae_lr_hip.so (explicitness_from_table)."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_dci_arguments(n, None, lat_sizes, n_train, n_test, seed, None, 1)
        _check_fit(fit, n_train, None, lat_sizes)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return explicitness_from_table(mean, lat_sizes, n_train=n_train, n_test=n_test, seed=seed,
                                       **({} if fit == "host" else {"fit": fit}))       # the default hands on what it always did

    def compute_infoe(self, dataloader, n_train=10000, n_test=5000, C=1.0, standardize=True, seed=0, rows=None):
        """InfoE of the model's representation (Hsu et al. 2023; infoe_from_table below, on the posterior means of the whole data set
        through the native encoder).  The data-set requirements and errors of compute_factor_scores; every size and argument is
        checked before any device work; train / eval mode is restored."""
        _ds, lat_sizes, n = self._factor_sizes(dataloader)
        _check_infoe_arguments(n, None, lat_sizes, n_train, n_test, C, seed, rows)
        mean, _logvar = self._encode(dataloader, n, lat_sizes)
        return infoe_from_table(mean, lat_sizes, n_train=n_train, n_test=n_test, C=C, standardize=standardize, seed=seed, rows=rows)

    # ------------------------------------------------------------------ MIG / AAM (evaluate.py:119-317)
    def compute_metrics(self, dataloader, sample_idx=None, n_samples=10000):
        """Mutual Information Gap and Axis Alignment Metric of the model on a data set with known, balanced factors of
        variation (evaluate.py:119-158): ``dataloader.dataset`` must expose ``lat_sizes`` / ``lat_names`` and the loader
        must iterate the data set in factor order (``shuffle=False``), as the reference requires.  Returns
        ``{'MIG': ..., 'AAM': ...}`` and writes the reference's ``metric_helpers.pth``.
        sample_idx: optional sequence of injected ``randperm`` draws (parity tests): the marginal one first, then one per
        (factor, value) in the reference's loop order."""
        ds, lat_sizes, n = self._factor_sizes(dataloader)
        draws = iter(sample_idx) if sample_idx is not None else None
        take = (lambda: None) if draws is None else (lambda: next(draws))
        self.logger.info("Computing the empirical distribution q(z|x).")
        table = _LatentTable(*self._encode(dataloader, n, lat_sizes))
        self.logger.info("Estimating the marginal entropy.")
        H_z = self._entropies(table, None, n_samples, take())                      # H[z_j]                 [D]
        H_zCv = torch.zeros(len(lat_sizes), table.dim, device=self.device)         # H[z_j | v_k]           [K, D]
        for k, (size, name) in enumerate(zip(lat_sizes, ds.lat_names)):
            for value in range(size):
                self.logger.info("Estimating conditional entropies for the {}th value of {}.".format(value, name))
                rows = table.rows_where(lat_sizes, k, value)
                H_zCv[k] += self._entropies(table, rows, n_samples, take()) / size
        scores = disentanglement_scores(H_z.cpu(), H_zCv.cpu(), lat_sizes)
        os.makedirs(self.save_dir, exist_ok=True)
        torch.save(scores, os.path.join(self.save_dir, METRIC_HELPERS_FILE))        # same keys as evaluate.py:151-156
        return {'MIG': scores["mig"].item(), 'AAM': scores["aam"].item()}

    @staticmethod
    def _factor_sizes(dataloader):
        """(data set, lat_sizes as ints, the number of images a data set that enumerates them holds) of a loader whose data set
        has known factors of variation."""
        ds = getattr(dataloader, "dataset", None)
        if not (hasattr(ds, "lat_sizes") and hasattr(ds, "lat_names")):
            raise ValueError("Dataset needs to have known true factors of variations to compute the metric. This does not "
                             "seem to be the case for {}".format(type(ds).__name__))
        lat_sizes = [int(k) for k in ds.lat_sizes]
        return ds, lat_sizes, int(np.prod(lat_sizes))            # (no factor: 1; every _check_* refuses that before it reads n)

    def _encode(self, dataloader, n=None, lat_sizes=None):
        """_encode_dataset in eval mode, train / eval mode restored.  n: the data set must tell that length, where it tells one
        (checked before the encoder runs), and the loader must yield that many images."""
        ds = getattr(dataloader, "dataset", None)
        if n is not None and hasattr(ds, "__len__") and len(ds) != n:
            raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (len(ds), lat_sizes))
        was_training = self.model.training
        self.model.eval()
        try:
            mean, logvar = self._encode_dataset(dataloader)
        finally:
            if was_training:
                self.model.train()
        if n is not None and mean.shape[0] != n:
            raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (mean.shape[0], lat_sizes))
        return mean, logvar

    def _encode_dataset(self, dataloader):
        """(mean, logvar) of q(z|x) for every image of the data set, [N, D] each on the device, through the native encoder
        (evaluate.py:196-231; in eval mode -- Evaluator.__call__ -- the reference's "sample" of q(z|x) is its mean,
        vae.py:69-71, so the table of means doubles as the table of samples)."""
        chunks = []
        with torch.no_grad():
            for x, _label in dataloader:
                chunks.append(self.model.encoder(x.to(self.device)))
        return torch.cat([m for m, _ in chunks]), torch.cat([lv for _, lv in chunks])

    def _entropies(self, table, rows, n_samples, draw):
        """H[z_j] = E_z[-log q(z_j)] with q(z_j) = 1/N sum_n q(z_j | x_n) over the `rows` of the table (None: all of it),
        estimated on n_samples of its own samples (evaluate.py:233-297), as one dvae_latent_entropy launch sequence.
        draw: the ``randperm(N)[:n_samples]`` of evaluate.py:259, or None to draw it here.  The reference re-views the
        gathered [n_samples, D] block as [D, n_samples] (:262, a reshape, not a transpose): the gathered block is handed to
        the kernel as that [D, S] image, which reproduces it exactly."""
        mean, logvar = table.select(rows)
        n, dim = mean.shape
        if draw is None:
            draw = torch.randperm(n, device=mean.device)
        draw = draw.to(mean.device)[:n_samples]
        if draw.numel() != n_samples:              # the reference's .view(latent_dim, n_samples) fails the same way
            raise RuntimeError("shape '[{}, {}]' is invalid for input of size {}".format(dim, n_samples, draw.numel() * dim))
        z_ds = mean.index_select(0, draw).contiguous()
        need = _lib.lib().dvae_latent_entropy_ws_floats(n, dim, n_samples)
        ws = getattr(self, "_metric_ws", None)
        if ws is None or ws.numel() < need or ws.device != mean.device:
            ws = self._metric_ws = torch.empty(need, dtype=torch.float32, device=mean.device)
        H = torch.empty(dim, dtype=torch.float32, device=mean.device)
        call("dvae_latent_entropy", ptr(z_ds), ptr(mean), ptr(logvar), n, dim, n_samples, ptr(ws), ptr(H), _stream())
        return H


class _LatentTable:
    """q(z|x) of a whole data set: mean / logvar [N, D] on the device, rows in the data set's factor order."""

    def __init__(self, mean, logvar):
        self.mean, self.logvar = mean.contiguous(), logvar.contiguous()
        self.n, self.dim = self.mean.shape
        self._index = None

    def rows_where(self, lat_sizes, factor, value):
        """Row numbers of the images whose `factor`-th factor of variation takes its `value`-th value, in data-set order
        (= the order of the reference's ``samples_zCx[..., value, ...]`` slice flattened, evaluate.py:311-314)."""
        if self._index is None:
            self._index = torch.arange(self.n, device=self.mean.device).view(*lat_sizes)
        return self._index.select(factor, value).reshape(-1)

    def select(self, rows):
        if rows is None:
            return self.mean, self.logvar
        return self.mean.index_select(0, rows), self.logvar.index_select(0, rows)


def disentanglement_scores(H_z, H_zCv, lat_sizes):
    """MIG (evaluate.py:160-180) and AAM (:182-194) from the marginal entropies H_z [D] and the conditional entropies
    H_zCv [K, D] of K balanced factors of variation (H[v_k] = log |V_k|).  I[z_j; v_k] = H[z_j] - H[z_j | v_k], negative
    estimates count as 0; per factor: MIG_k = (largest - second largest information) / H[v_k], AAM_k = max(0, largest -
    all the others) / largest (0 where no latent carries information).  Returns the reference's metric_helpers dict."""
    info = (H_z.unsqueeze(0) - H_zCv).clamp(min=0)                 # [K, D]
    ranked = torch.sort(info, dim=1, descending=True)[0]
    best, runner_up = ranked[:, 0], ranked[:, 1] if ranked.shape[1] > 1 else torch.zeros_like(ranked[:, 0])
    mig_k = (best - runner_up) / torch.tensor([float(k) for k in lat_sizes]).log()
    others = ranked[:, 1:].sum(dim=1)
    aam_k = torch.where(best > 0, (best - others).clamp(min=0) / best, torch.zeros_like(best))
    return {"marginal_entropies": H_z, "cond_entropies": H_zCv, "mig_k": mig_k, "mig": mig_k.mean(),
            "aam_k": aam_k, "aam": aam_k.mean()}


def separability_scores_from_entropies(H_z, H_z_d, H_loo, H_cond_d):
    """The scores of Do & Tran 2020 from entropies under the aggregate posterior, combined in fp64 (python floats; arrays come
    back as lists): H_z = H(z), H_z_d[i] = H(z_i), H_loo[i] = H(z_!=i) (D = 1: 0), H_cond_d[i] = H(z_i | x).  q(z|x) is factorised,
    so H(z_A | x) = sum_{d in A} H_cond_d[d]:

        informativeness[i] = I(x; z_i)        = H_z_d[i] - H_cond_d[i]
        mi                 = I(x; z)          = H_z - sum_d H_cond_d[d]
        mi_loo[i]          = I(x; z_!=i)      = H_loo[i] - sum_{d != i} H_cond_d[d]
        sepin[i]           = I(x; z_i | z_!=i) = mi - mi_loo[i]
        redundancy[i]      = I(z_i; z_!=i)    = H_z_d[i] + H_loo[i] - H_z            (sepin = informativeness - redundancy)
        rho[i]             = max(informativeness[i], 0) / sum_j max(informativeness[j], 0)      (all zero: rho = 0, wsepin = 0)
        wsepin             = sum_i rho[i] sepin[i]
        sepin_at_k[k-1]    = mean of the k largest sepin[i]
        dtc                = sum_i H_loo[i] - (D - 1) H_z      (dual total correlation);  tc = sum_i H_z_d[i] - H_z

    Nothing is clamped except inside rho: these are estimates and may come out slightly negative."""
    H_z = float(H_z)
    H_z_d, H_loo, H_cond_d = ([float(v) for v in h] for h in (H_z_d, H_loo, H_cond_d))
    dim = len(H_z_d)
    if dim < 1 or len(H_loo) != dim or len(H_cond_d) != dim:
        raise ValueError("H_z_d, H_loo and H_cond_d must hold one entropy per latent dimension, got %d, %d and %d"
                         % (dim, len(H_loo), len(H_cond_d)))
    informativeness = [H_z_d[i] - H_cond_d[i] for i in range(dim)]
    mi = H_z - math.fsum(H_cond_d)
    mi_loo = [H_loo[i] - math.fsum(H_cond_d[:i] + H_cond_d[i + 1:]) for i in range(dim)]
    sepin = [mi - mi_loo[i] for i in range(dim)]
    redundancy = [H_z_d[i] + H_loo[i] - H_z for i in range(dim)]
    weight = [max(v, 0.0) for v in informativeness]
    total = math.fsum(weight)
    rho = [w / total for w in weight] if total > 0.0 else [0.0] * dim
    wsepin = math.fsum(r * v for r, v in zip(rho, sepin))
    ranked = sorted(sepin, reverse=True)
    sepin_at_k = [math.fsum(ranked[:k]) / k for k in range(1, dim + 1)]
    return {"sepin": sepin, "wsepin": wsepin, "sepin_at_k": sepin_at_k, "informativeness": informativeness, "redundancy": redundancy,
            "rho": rho, "mi": mi, "mi_loo": mi_loo, "dtc": math.fsum(H_loo) - (dim - 1) * H_z, "tc": math.fsum(H_z_d) - H_z}


# ---------------------------------------------------------------------- lines that the _check_* functions below share
def _check_lat_sizes(lat_sizes, max_factors=None):
    if len(lat_sizes) < 1 or min(lat_sizes) < 1:
        raise ValueError("lat_sizes must hold positive sizes, got %s" % (lat_sizes,))
    if max_factors is not None and len(lat_sizes) > max_factors:
        raise ValueError("%d factors of variation: the kernels take at most %d" % (len(lat_sizes), max_factors))


def _check_n_samples(n, n_samples):
    if n_samples is not None and not 1 <= int(n_samples) <= n:
        raise ValueError("n_samples must lie in [1, %d] (rows are drawn without replacement) or be None, got %r" % (n, n_samples))


# ---------------------------------------------------------------------- FactorVAE / beta-VAE scores on a table of means
def _check_score_sizes(n, lat_sizes, n_train, n_eval, batch_size, n_variance):
    _check_lat_sizes(lat_sizes)
    if max(lat_sizes) < 2:
        raise ValueError("no factor of variation takes two values or more: lat_sizes=%s" % (lat_sizes,))
    if int(n_train) < 1 or int(n_eval) < 1:
        raise ValueError("n_train and n_eval must be >= 1, got %r and %r" % (n_train, n_eval))
    if int(batch_size) < 2:
        raise ValueError("batch_size must be >= 2 (a variance needs two points), got %r" % (batch_size,))
    if min(n, int(n_variance)) < 2:
        raise ValueError("the global variance needs two rows or more: n_variance=%r on %d images" % (n_variance, n))


def draw_fixed_factor_rows(lat_sizes, n_groups, batch_size, generator, device="cpu", paired=False):
    """Rows of a data set that enumerates ``lat_sizes`` in row-major order, drawn in ``n_groups`` groups of ``batch_size``
    with one factor of variation held fixed.  Per group a factor k is drawn uniformly among the factors with two values or
    more; every member gets independent uniform values of every factor (with replacement: N never limits the group), and
    column k is then overwritten --

    * paired=False (FactorVAE): with ONE value per group.  Returns (factor int32 [V], rows int64 [V, L]).
    * paired=True (beta-VAE): a second, independent set of values is drawn for the b side and the a side's column k is copied
      into it member by member (each PAIR shares its value).  Returns (factor, rows_a, rows_b).

    A row is sum_j value_j * stride_j.  All draws come from ``generator`` (a torch.Generator of ``device``)."""
    sizes = [int(k) for k in lat_sizes]
    V, L, K = int(n_groups), int(batch_size), len(sizes)
    eligible = [k for k, size in enumerate(sizes) if size >= 2]
    if not eligible:
        raise ValueError("no factor of variation takes two values or more: lat_sizes=%s" % (sizes,))
    strides = [int(np.prod(sizes[j + 1:])) for j in range(K)]
    opts = dict(generator=generator, device=device)

    def uniform_values(*shape):
        return torch.stack([torch.randint(size, shape, **opts) for size in sizes], dim=-1)          # [..., K] int64

    pick = torch.randint(len(eligible), (V,), **opts)
    factor = torch.tensor(eligible, dtype=torch.int64, device=device)[pick]                         # [V]
    column = factor.view(V, 1, 1).expand(V, L, 1)
    values = uniform_values(V, L)
    stride_t = torch.tensor(strides, dtype=torch.int64, device=device)
    if not paired:
        fixed = uniform_values(V).gather(1, factor.view(V, 1))                                      # [V, 1]: one value per group
        values.scatter_(2, column, fixed.view(V, 1, 1).expand(V, L, 1))
        return factor.to(torch.int32), (values * stride_t).sum(-1).contiguous()
    values_b = uniform_values(V, L)
    values_b.scatter_(2, column, values.gather(2, column))
    return factor.to(torch.int32), (values * stride_t).sum(-1).contiguous(), (values_b * stride_t).sum(-1).contiguous()


def fit_logistic_regression(features, labels, n_classes, C=1.0, max_iter=500, tolerance_grad=1e-8):
    """Multinomial logistic regression in fp64 on the CPU: minimise mean cross-entropy + ||W||^2 / (2 C n) with an unpenalised
    bias (sklearn's default objective) from zero, by L-BFGS with a strong-Wolfe line search until the largest absolute gradient
    entry is below ``tolerance_grad`` or ``max_iter`` iterations have passed.  features [n, D], labels [n] in [0, n_classes).
    Returns (W [n_classes, D], b [n_classes]) as fp64 tensors.  The objective is strictly convex in W: the optimum is unique."""
    X = torch.as_tensor(features, dtype=torch.float64, device="cpu")
    y = torch.as_tensor(labels, dtype=torch.int64, device="cpu")
    n, dim = X.shape
    W = torch.zeros(n_classes, dim, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(n_classes, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([W, b], lr=1.0, max_iter=int(max_iter), max_eval=25 * int(max_iter), tolerance_grad=tolerance_grad,
                            tolerance_change=0.0, history_size=100, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(X @ W.t() + b, y) + (W * W).sum() / (2.0 * C * n)
        loss.backward()
        return loss
    opt.step(closure)
    return W.detach(), b.detach()


def _classifier_accuracy(W, b, classes, features, labels):
    """Share of rows whose arg-max logit (the lowest class on ties) is their label; classes[i] = the label of logit i."""
    logits = torch.as_tensor(features, dtype=torch.float64) @ W.t() + b
    pred = classes[torch.argmax(logits, dim=1)]
    return float((pred == labels).double().mean().item())


def factor_scores_from_table(mean, lat_sizes, n_train=10000, n_eval=5000, batch_size=64, n_variance=10000,
                             active_threshold=0.05, seed=0, draws=None, return_details=False, fit="host"):
    """FactorVAE score and beta-VAE score of a representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data
    set that enumerates ``lat_sizes`` in row-major order.

    FactorVAE: var = unbiased variance per dimension over min(N, n_variance) rows drawn without replacement
    (dvae_score_group_var, one group); active[d] = sqrt(var[d]) >= active_threshold.  For the train and the eval set: groups
    of ``batch_size`` rows with one factor fixed (draw_fixed_factor_rows), their variance per dimension divided by var
    (dvae_score_group_var), the active dimension with the smallest value votes for the group's factor (dvae_score_vote).  The
    classifier is c[d] = argmax_k votes_train[k, d] (the lowest k on ties); factor_vae_train = sum_d max_k votes_train[k, d] /
    n_train, factor_vae_eval = sum_d votes_eval[c[d], d] / n_eval; both 0 without an active dimension.

    beta-VAE: per group of ``batch_size`` PAIRS that share one factor's value the mean |z_a - z_b| per dimension
    (dvae_score_pair_absdiff) is one feature vector labelled with the factor; fit_logistic_regression on the train set (classes
    = the factors that occur in it), the scores are its accuracies on the train and the eval features.

    Draws come from a private generator seeded with ``seed`` (the same seed gives the same bits, the global random states are
    untouched).  ``draws`` injects them, each key on its own: "variance_rows" ([n] rows), "factor_vae_train" /
    "factor_vae_eval" ((factor, rows)), "beta_vae_train" / "beta_vae_eval" ((factor, rows_a, rows_b)); injected rows and
    factors are range-checked here (the kernels do not).  return_details=True: (scores, details) with the host copies of var,
    active, the vote matrices, the classifier, the beta-VAE features / labels and (W, b).
    fit="device": the beta-VAE classifier is fitted where its features lie (dvae_lr_fit of libdvae_lr_hip.so, the same objective
    to tolerance_grad 1e-8; a fit that does not get there raises DvaeHipError) and its accuracies are dvae_lr_predict's counts
    of correct rows; n_train <= 16384 and D <= 64 then."""
    lat_sizes = [int(k) for k in lat_sizes]
    K = len(lat_sizes)
    if mean.dim() != 2:
        raise ValueError("mean must be an [N, D] table, got shape %s" % (tuple(mean.shape),))
    n, dim = int(mean.shape[0]), int(mean.shape[1])
    _check_score_sizes(n, lat_sizes, n_train, n_eval, batch_size, n_variance)
    _check_fit(fit, n_train, dim, [K])
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if dim < 1:
        raise ValueError("mean must have one latent dimension or more")
    if not mean.is_cuda:
        raise _lib.DvaeHipError("factor_scores_from_table needs the table on the GPU (there is no CPU / PyTorch fallback for "
                                "the score kernels)")
    n_train, n_eval, L = int(n_train), int(n_eval), int(batch_size)
    dev = mean.device
    table = mean.detach().to(torch.float32).contiguous()
    draws = dict(draws or {})
    unknown = set(draws) - {"variance_rows", "factor_vae_train", "factor_vae_eval", "beta_vae_train", "beta_vae_eval"}
    if unknown:
        raise ValueError("unknown draws: %s" % sorted(unknown))
    gen = torch.Generator(device=dev).manual_seed(int(seed))

    def rows_of(t, shape=None):
        t = torch.as_tensor(t).to(dev, torch.int64).contiguous()
        if (shape is not None and tuple(t.shape) != shape) or t.numel() == 0 or not (0 <= int(t.min()) and int(t.max()) < n):
            raise ValueError("injected rows must have shape %s and lie in [0, %d)" % (shape, n))
        return t

    def factor_of(t, V):
        t = torch.as_tensor(t).to(dev, torch.int32).contiguous()
        if tuple(t.shape) != (V,) or not (0 <= int(t.min()) and int(t.max()) < K):
            raise ValueError("injected factors must have shape (%d,) and lie in [0, %d)" % (V, K))
        return t

    def drawn(key, V, paired):
        if key in draws:
            got = draws[key]
            if len(got) != (3 if paired else 2):
                raise ValueError("draws[%r] must be %s" % (key, "(factor, rows_a, rows_b)" if paired else "(factor, rows)"))
            return (factor_of(got[0], V),) + tuple(rows_of(r, (V, L)) for r in got[1:])
        return draw_fixed_factor_rows(lat_sizes, V, L, gen, device=dev, paired=paired)

    S = _scorelib.lib()
    st = _stream()

    def group_var(rows, inv_scale):
        V, Lg = rows.shape
        ws = torch.empty(max(S.dvae_score_group_var_ws_floats(n, dim, V, Lg), 1), dtype=torch.float32, device=dev)
        out = torch.empty(V, dim, dtype=torch.float32, device=dev)
        _scorelib.call("dvae_score_group_var", ptr(table), ptr(rows), n, dim, V, Lg, ptr(inv_scale), ptr(ws), ptr(out), st)
        return out

    # ---- FactorVAE
    if "variance_rows" in draws:
        var_rows = rows_of(draws["variance_rows"]).view(1, -1)
        if var_rows.shape[1] < 2:
            raise ValueError("the global variance needs two rows or more")
    else:
        var_rows = torch.randperm(n, generator=gen, device=dev)[:min(n, int(n_variance))].contiguous().view(1, -1)
    var_dev = group_var(var_rows, None).view(dim)
    var = var_dev.cpu().numpy()                                                        # [D] fp32 -> host
    active = np.sqrt(var.astype(np.float64)) >= float(active_threshold)
    active_dev = torch.from_numpy(active.astype(np.int32)).to(dev)
    inv_scale = (1.0 / var_dev).contiguous()
    votes = {}
    for key, V in (("train", n_train), ("eval", n_eval)):
        factor, rows = drawn("factor_vae_" + key, V, paired=False)
        stat = group_var(rows, inv_scale)
        argmin = torch.empty(V, dtype=torch.int32, device=dev)
        votes[key] = torch.empty(K, dim, dtype=torch.int32, device=dev)
        _scorelib.call("dvae_score_vote", ptr(stat), ptr(factor), ptr(active_dev), V, dim, K, ptr(argmin), ptr(votes[key]), st)
    votes_train, votes_eval = votes["train"].cpu().numpy().astype(np.int64), votes["eval"].cpu().numpy().astype(np.int64)
    classifier = votes_train.argmax(axis=0)                                            # [D], the lowest k on ties
    factor_vae_train = float(votes_train.max(axis=0).sum()) / n_train
    factor_vae_eval = float(votes_eval[classifier, np.arange(dim)].sum()) / n_eval

    # ---- beta-VAE
    feats, labels = {}, {}
    for key, V in (("train", n_train), ("eval", n_eval)):
        factor, rows_a, rows_b = drawn("beta_vae_" + key, V, paired=True)
        out = torch.empty(V, dim, dtype=torch.float32, device=dev)
        _scorelib.call("dvae_score_pair_absdiff", ptr(table), ptr(rows_a), ptr(rows_b), n, dim, V, L, ptr(out), st)
        feats[key], labels[key] = out, factor
    if fit == "device":
        return _beta_vae_on_the_device(feats, labels, factor_vae_train, factor_vae_eval, active, n_train, n_eval, L, st, return_details,
                                       {"var": var, "active": active, "votes_train": votes_train, "votes_eval": votes_eval,
                                        "classifier": classifier})
    feats = {k: v.cpu().double() for k, v in feats.items()}
    labels = {k: v.cpu().to(torch.int64) for k, v in labels.items()}
    classes = torch.unique(labels["train"])                                            # sorted
    if classes.numel() > 1:
        W, b = fit_logistic_regression(feats["train"], torch.searchsorted(classes, labels["train"]), classes.numel())
    else:                                                                              # one class: nothing to fit
        W, b = torch.zeros(1, dim, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    scores = {"factor_vae_train": factor_vae_train, "factor_vae_eval": factor_vae_eval,
              "beta_vae_train": _classifier_accuracy(W, b, classes, feats["train"], labels["train"]),
              "beta_vae_eval": _classifier_accuracy(W, b, classes, feats["eval"], labels["eval"]),
              "n_active": int(active.sum()), "n_train": n_train, "n_eval": n_eval, "batch_size": L}
    if not return_details:
        return scores
    return scores, {"var": var, "active": active, "votes_train": votes_train, "votes_eval": votes_eval, "classifier": classifier,
                    "features_train": feats["train"], "features_eval": feats["eval"], "labels_train": labels["train"],
                    "labels_eval": labels["eval"], "classes": classes, "W": W, "b": b}


# ---------------------------------------------------------------------- shared by the scores on a table of means
def _table_shape(mean):
    if mean.dim() != 2:
        raise ValueError("mean must be an [N, D] table, got shape %s" % (tuple(mean.shape),))
    return int(mean.shape[0]), int(mean.shape[1])


def _checked_rows(rows, n):
    """An injected selection -> int64 [S], S >= 1, every row number in [0, n): the kernels do not check them."""
    rows = torch.as_tensor(rows).to(torch.int64).reshape(-1)
    if rows.numel() < 1 or not (0 <= int(rows.min()) and int(rows.max()) < n):
        raise ValueError("rows must hold one row number or more, each in [0, %d)" % n)
    return rows


def _select_rows(mean, rows, n_samples, seed, caller, kernels):
    """What the *_from_table functions do once their own arguments are checked, in this order: ``rows`` is validated, the table
    must be finite, then on the GPU.  -> (table fp32 contiguous, rows int64 on the device or None for every row, S, device);
    rows=None and n_samples given: randperm(N)[:n_samples] from a private generator seeded with ``seed``."""
    n = int(mean.shape[0])
    if rows is not None:
        rows = _checked_rows(rows, n)
    if not bool(torch.isfinite(mean).all()):
        raise ValueError("the table of means holds a NaN or an infinity")
    if not mean.is_cuda:
        raise _lib.DvaeHipError("%s needs the table on the GPU (there is no CPU / PyTorch fallback for the %s kernels)" % (caller, kernels))
    dev = mean.device
    table = mean.detach().to(torch.float32).contiguous()
    if rows is not None:
        rows = rows.to(dev).contiguous()
    elif n_samples is not None:
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        rows = torch.randperm(n, generator=gen, device=dev)[:int(n_samples)].contiguous()
    return table, rows, n if rows is None else int(rows.numel()), dev


def mutual_information_from_counts(block):
    """fp64 [B, R, C] integer-valued joint counts of B tables over the same S rows -> mutual information [B] in nats:
    sum over the nonzero cells of P log(P / (P_row P_col)), P = counts / S (sklearn's mutual_info_score)."""
    S = block[0].sum()
    row, col = block.sum(axis=2, keepdims=True), block.sum(axis=1, keepdims=True)
    # P / (P_row P_col) = c S / (row col) from the integer counts: both products are exact in fp64, so a cell of an independent
    # table (a constant or collapsed latent: row = S) contributes log(1) = 0 exactly and modularity's "t = 0" sees the number 0
    nz = block > 0
    term = np.zeros_like(block)
    term[nz] = block[nz] / S * np.log((block * S)[nz] / (row * col)[nz])
    return term.sum(axis=(1, 2))


# ---------------------------------------------------------------------- discretised MIG / modularity / SAP on a table of means
def _check_information_sizes(n, lat_sizes, n_bins, n_samples):
    _check_lat_sizes(lat_sizes, _infolib.MAX_FACTORS)
    if not 1 <= int(n_bins) <= _infolib.MAX_BINS:
        raise ValueError("n_bins must lie in [1, %d], got %r" % (_infolib.MAX_BINS, n_bins))
    if min(lat_sizes) < 2:
        raise ValueError("a factor of variation with one value has no entropy (the MIG divides by it): lat_sizes=%s" % (lat_sizes,))
    _check_n_samples(n, n_samples)


def histogram_edges(lo, hi, n_bins):
    """The n_bins lower bin edges numpy.histogram(x, n_bins) uses for an fp32 column with minimum lo and maximum hi, bit for bit:
    numpy's own linspace between the two np.float32 scalars (a constant column: lo - 0.5 and hi + 0.5, as numpy does).  The same
    edges formed from Python floats differ in the last bit for most columns.  Where numpy refuses (a range of fewer than n_bins
    ulps) neighbouring edges coincide; the bin of x stays defined as the number of edges <= x, minus one."""
    lo, hi = np.float32(lo), np.float32(hi)
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(0.5)), np.float32(hi + np.float32(0.5))
    return np.linspace(lo, hi, int(n_bins) + 1, dtype=np.float32)[:-1]


def largest_gap(m):
    """[D, K] -> the largest minus the second largest entry over d, [K]; one latent: the second largest counts as 0."""
    ranked = np.sort(m, axis=0)[::-1]
    return ranked[0] - (ranked[1] if m.shape[0] > 1 else 0.0)


def information_scores_from_statistics(counts, lat_sizes, n_bins, col_var, factor_var, cov_zv):
    """The host half of information_scores_from_table, fp64: ``counts`` int [D, n_bins * sum(lat_sizes)] in the layout of
    dvae_info_joint_hist, col_var [D], factor_var [K], cov_zv [D, K] of dvae_info_moments.

    mutual_information[d, k] = sum over the nonzero cells of P log(P / (P_row P_col)), P = counts / S (nats; sklearn's
    mutual_info_score); factor_entropy[k] = entropy of factor k's values among the selected rows;
    mig_discrete = mean_k (largest - second largest MI over d) / factor_entropy[k] (one latent: the second is 0; a factor without
    entropy raises ValueError);  modularity = mean_d [1 - (sum m - t) / (t (K - 1))], m = MI[d, :]^2, t = max m (0 where t = 0;
    K = 1: 1 where t > 0);  sap_matrix[d, k] = cov_zv^2 / (col_var factor_var) where col_var > 1e-12, else 0;
    sap_continuous = mean_k (largest - second largest over d)."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_bins = len(lat_sizes), int(n_bins)
    counts = np.asarray(counts).astype(np.int64)
    D = counts.shape[0]
    assert counts.shape == (D, n_bins * sum(lat_sizes)), counts.shape
    mi, H = np.zeros((D, K)), np.zeros(K)
    start = 0
    for k, size in enumerate(lat_sizes):
        block = counts[:, start:start + n_bins * size].reshape(D, n_bins, size).astype(np.float64)
        start += n_bins * size
        mi[:, k] = mutual_information_from_counts(block)
        pv = block[0].sum(axis=0) / block[0].sum()                       # the factor's values among the selected rows: any d
        H[k] = -(pv[pv > 0] * np.log(pv[pv > 0])).sum()
    if not (H > 0).all():
        raise ValueError("factor(s) %s take one value among the selected rows: no entropy to divide the MIG by"
                         % [k for k in range(K) if not H[k] > 0])

    gap = largest_gap
    m = mi ** 2
    t = m.max(axis=1)
    modularity_d = np.zeros(D)
    if K > 1:
        modularity_d[t > 0] = 1.0 - (m.sum(axis=1) - t)[t > 0] / (t[t > 0] * (K - 1))
    else:
        modularity_d[t > 0] = 1.0
    col_var, factor_var, cov_zv = (np.asarray(a, dtype=np.float64) for a in (col_var, factor_var, cov_zv))
    sap = np.zeros((D, K))
    live = col_var > 1e-12
    sap[live] = cov_zv[live] ** 2 / (col_var[live, None] * factor_var[None, :])
    return {"mig_discrete": float(np.mean(gap(mi) / H)), "modularity": float(modularity_d.mean()),
            "sap_continuous": float(np.mean(gap(sap))), "sap_matrix": sap, "mutual_information": mi, "factor_entropy": H}


def information_scores_from_table(mean, lat_sizes, n_bins=20, n_samples=None, seed=0, rows=None):
    """Discretised MIG, modularity and continuous-factor SAP of a representation given as the fp32 [N, D] table ``mean`` (on the
    GPU) of a data set that enumerates ``lat_sizes`` in row-major order (formulas: information_scores_from_statistics).

    n_samples=None: every row; else rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed
    gives the same bits, the global random states are untouched); ``rows`` ([S] row numbers in [0, N), repeats allowed) injects
    the selection.  Every size and argument is checked before any device work, and a table with a NaN or an infinity raises
    ValueError.  dvae_info_moments, ONE device-to-host copy of its outputs, the bin edges of numpy.histogram on the host
    (histogram_edges), dvae_info_joint_hist, ONE copy of the counts, the scores in fp64 on the host.  Returns {"mig_discrete",
    "modularity", "sap_continuous", "sap_matrix" [D, K], "mutual_information" [D, K], "factor_entropy" [K], "n_samples",
    "n_bins"}: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_bins = len(lat_sizes), int(n_bins)
    n, dim = _table_shape(mean)
    _check_information_sizes(n, lat_sizes, n_bins, None if rows is not None else n_samples)
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if dim < 1:
        raise ValueError("mean must have one latent dimension or more")
    table, rows, S, dev = _select_rows(mean, rows, n_samples, seed, "information_scores_from_table", "information-score")
    I = _infolib.lib()
    st = _stream()
    sizes_dev = torch.tensor(lat_sizes, dtype=torch.int32, device=dev)
    sum_sizes = sum(lat_sizes)
    ws = torch.empty(max(I.dvae_info_moments_ws_floats(n, dim, K, S), I.dvae_info_hist_ws_floats(n, dim, K, S, n_bins, sum_sizes), 1),
                     dtype=torch.float32, device=dev)
    out = torch.empty(4 * dim + dim * K + 2 * K, dtype=torch.float32, device=dev)
    parts = torch.split(out, [dim, dim, dim, dim, dim * K, K, K])
    _infolib.call("dvae_info_moments", ptr(table), ptr(rows), ptr(sizes_dev), n, dim, K, S, ptr(ws), *[ptr(p) for p in parts], st)
    col_min, col_max, _col_mean, col_var, cov_zv, _factor_mean, factor_var = (p.numpy() for p in torch.split(
        out.cpu(), [dim, dim, dim, dim, dim * K, K, K]))                               # ONE device->host copy
    edges = np.stack([histogram_edges(col_min[d], col_max[d], n_bins) for d in range(dim)])
    edges_dev = torch.from_numpy(edges).to(dev)
    counts = torch.empty(dim, n_bins * sum_sizes, dtype=torch.int32, device=dev)
    _infolib.call("dvae_info_joint_hist", ptr(table), ptr(rows), ptr(sizes_dev), ptr(edges_dev), n, dim, K, S, n_bins, sum_sizes,
                  ptr(ws), ptr(counts), st)
    scores = information_scores_from_statistics(counts.cpu().numpy(), lat_sizes, n_bins, col_var, factor_var,
                                                cov_zv.reshape(dim, K))               # ONE copy of the counts
    scores.update(n_samples=S, n_bins=n_bins)
    return scores


# ---------------------------------------------------------------------- RMIG / JEMMIG / MIG-sup / DCIMIG on the posterior mass table
def _check_interpretability_arguments(n, lat_sizes, n_bins, z_range, n_samples, dim=None):
    _check_lat_sizes(lat_sizes, _masslib.MAX_FACTORS)
    if not 1 <= int(n_bins) <= _masslib.MAX_BINS:
        raise ValueError("n_bins must lie in [1, %d], got %r" % (_masslib.MAX_BINS, n_bins))
    if len(z_range) != 2 or not (math.isfinite(z_range[0]) and math.isfinite(z_range[1]) and float(z_range[0]) < float(z_range[1])):
        raise ValueError("z_range must be (lo, hi), finite, lo < hi, got %r" % (z_range,))
    if min(lat_sizes) < 2:
        raise ValueError("a factor of variation with one value has no entropy (the scores divide by it): lat_sizes=%s" % (lat_sizes,))
    if dim is not None and not (1 <= dim <= 16384 and dim * int(n_bins) * sum(lat_sizes) <= 2 ** 31 - 1):
        raise ValueError("%d latent dimensions x %d bins x %d factor values: the mass table is limited to 16384 dimensions and "
                         "2^31 - 1 elements" % (dim, n_bins, sum(lat_sizes)))
    _check_n_samples(n, n_samples)


def mass_edges(n_bins, z_range=(-4., 4.)):
    """The n_bins - 1 inner bin edges, fp64: numpy.linspace(lo, hi, n_bins + 1)[1:-1].  Bin 0 reaches down to -inf and bin
    n_bins - 1 up to +inf, so the tails outside z_range are folded into the end bins and the masses of a row sum to 1."""
    return np.linspace(float(z_range[0]), float(z_range[1]), int(n_bins) + 1)[1:-1].astype(np.float64)


def interpretability_scores_from_mass(mass, lat_sizes, n_bins):
    """The host half of interpretability_scores_from_table, fp64: ``mass`` [D, n_bins * sum(lat_sizes)] in the layout of
    dvae_mass_joint -- for latent d and factor k the block [n_bins, lat_sizes[k]] of posterior mass per (bin, factor value),
    mass[d][k][b, v] = sum over the selected rows with v_k = v of Q_b(row, d).  Each block is normalised by its own sum: P.

    mutual_information[d, k] = sum P log(P / (P_z P_v)) and joint_entropy[d, k] = -sum P log P over the cells with P > 0 (nats; P_z
    the bin marginal, P_v the value marginal); factor_entropy[k] = H_y[k], the entropy of the value marginal of block (0, k) (a
    factor without entropy raises ValueError); latent_entropy[d] the entropy of the bin marginal of block (d, 0).
    Per factor k, with i* = arg max_d I[d, k] (the lowest d on ties; best_latent[k]) and j the runner-up (one latent: its MI is 0):
        rmig_per_factor[k] = I[i*, k] - I[j, k]                                  rmig_norm = mean_k rmig_per_factor[k] / H_y[k]
        jemmig_per_factor[k] = H_joint[i*, k] - I[i*, k] + I[j, k]               jemmig_norm_per_factor[k] = 1 - jemmig_k / (H_y[k] + log n_bins)
    (Do & Tran 2020).  Per latent d: mig_sup_per_latent[d] = largest - second largest over k of I[d, k] / H_y[k] (one factor: the
    second is 0; Li et al. 2020).  dcimig = sum_k max_{d : k(d) = k} gap_d / sum_k H_y[k] with k(d) = arg max_k I[d, k] and gap_d
    the largest minus the second largest of I[d, :] (a factor no latent prefers contributes 0; Sepliarskaia et al. 2019).
    rmig, rmig_norm, jemmig, jemmig_norm and mig_sup are the means of their arrays."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_bins = len(lat_sizes), int(n_bins)
    mass = np.asarray(mass, dtype=np.float64)
    D = mass.shape[0]
    if mass.ndim != 2 or D < 1 or mass.shape[1] != n_bins * sum(lat_sizes):
        raise ValueError("mass must be [D, n_bins * sum(lat_sizes)] = [D, %d], got shape %s" % (n_bins * sum(lat_sizes), mass.shape))

    def entropy(p):
        return float(-(p[p > 0] * np.log(p[p > 0])).sum())
    mi, joint, H_y, H_z = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(D)
    start = 0
    for k, size in enumerate(lat_sizes):
        for d in range(D):
            P = mass[d, start:start + n_bins * size].reshape(n_bins, size)
            P = P / P.sum()
            Pz, Pv = P.sum(axis=1, keepdims=True), P.sum(axis=0, keepdims=True)
            nz = P > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = P / Pz / Pv                                      # (P / P_z) / P_v: the PRODUCT of two marginals of 1e-200 is 0 where P is not
            mi[d, k] = (P[nz] * np.log(ratio[nz])).sum()
            joint[d, k] = entropy(P)
            if d == 0:
                H_y[k] = entropy(Pv)
            if k == 0:
                H_z[d] = entropy(Pz)
        start += n_bins * size
    if not (H_y > 0).all():
        raise ValueError("factor(s) %s take one value among the selected rows: no entropy to divide the scores by"
                         % [k for k in range(K) if not H_y[k] > 0])
    best = mi.argmax(axis=0)                                             # [K], the lowest d on ties
    top = mi[best, np.arange(K)]
    second = np.array([np.delete(mi[:, k], best[k]).max() if D > 1 else 0.0 for k in range(K)])
    rmig_k = top - second
    jemmig_k = joint[best, np.arange(K)] - top + second
    jemmig_norm_k = 1.0 - jemmig_k / (H_y + math.log(n_bins))
    ranked = np.sort(mi / H_y[None, :], axis=1)[:, ::-1]                 # [D, K], descending over k
    mig_sup_d = ranked[:, 0] - (ranked[:, 1] if K > 1 else 0.0)
    raw = np.sort(mi, axis=1)[:, ::-1]
    gap_d = raw[:, 0] - (raw[:, 1] if K > 1 else 0.0)
    prefers = mi.argmax(axis=1)                                          # [D], k(d)
    dcimig = sum(gap_d[prefers == k].max() for k in range(K) if (prefers == k).any()) / H_y.sum()
    return {"rmig": float(rmig_k.mean()), "rmig_norm": float((rmig_k / H_y).mean()), "jemmig": float(jemmig_k.mean()),
            "jemmig_norm": float(jemmig_norm_k.mean()), "mig_sup": float(mig_sup_d.mean()), "dcimig": float(dcimig),
            "rmig_per_factor": rmig_k, "jemmig_per_factor": jemmig_k, "jemmig_norm_per_factor": jemmig_norm_k,
            "mig_sup_per_latent": mig_sup_d, "best_latent": best.astype(np.int64), "factor_entropy": H_y, "latent_entropy": H_z,
            "mutual_information": mi, "joint_entropy": joint, "n_samples": int(round(float(mass[0, :n_bins * lat_sizes[0]].sum()))),
            "n_bins": n_bins}


def interpretability_scores_from_table(mean, logvar, lat_sizes, n_bins=100, z_range=(-4., 4.), n_samples=None, seed=0, rows=None):
    """RMIG, JEMMIG, MIG-sup and DCIMIG of a representation given as the fp32 [N, D] tables ``mean`` and ``logvar`` of q(z|x) (on
    the GPU) of a data set that enumerates ``lat_sizes`` in row-major order (formulas: interpretability_scores_from_mass).

    The posterior of every selected row is INTEGRATED over n_bins fixed bins with the inner edges mass_edges(n_bins, z_range),
    the tails beyond z_range folded into the end bins: with sigma = exp(logvar / 2), t_j = (e_j - mean) / (sigma sqrt 2),
    up_j = erfc(t_j) / 2 and dn_j = erfc(-t_j) / 2 in fp64, Q_0 = dn_1, Q_{n_bins-1} = up_{n_bins-1} and for the bins between
    Q_b = up_b - up_{b+1} if t_b >= 0 else dn_{b+1} - dn_b -- always the difference of the two smaller tails, never
    Phi(b) - Phi(a), which loses every small mass.  mass[d][k][b, v] is the sum of Q_b over the selected rows whose factor k
    takes the value v (dvae_mass_joint, fp64, fixed order).

    n_samples=None: every row; else rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed
    gives the same bits, the global random states are untouched); ``rows`` ([S] row numbers in [0, N), repeats allowed) injects
    the selection.  Every size and argument is checked before any device work, and a table with a NaN or an infinity raises
    ValueError.  ONE launch sequence, ONE device-to-host copy of the mass table, the scores in fp64 on the host.  Returns the
    dictionary of interpretability_scores_from_mass with n_samples = S: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_bins = len(lat_sizes), int(n_bins)
    n, dim = _table_shape(mean)
    if tuple(logvar.shape) != tuple(mean.shape):
        raise ValueError("logvar must have the shape of mean, %s, got %s" % (tuple(mean.shape), tuple(logvar.shape)))
    _check_interpretability_arguments(n, lat_sizes, n_bins, z_range, None if rows is not None else n_samples, dim=max(dim, 1))
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if dim < 1:
        raise ValueError("mean must have one latent dimension or more")
    if not bool(torch.isfinite(logvar).all()):
        raise ValueError("the table of log-variances holds a NaN or an infinity")
    table, rows, S, dev = _select_rows(mean, rows, n_samples, seed, "interpretability_scores_from_table", "posterior-mass")
    if logvar.device != dev:
        raise _lib.DvaeHipError("interpretability_scores_from_table needs mean and logvar on the same GPU")
    logvar = logvar.detach().to(torch.float32).contiguous()
    M = _masslib.lib()
    sum_sizes = sum(lat_sizes)
    sizes_dev = torch.tensor(lat_sizes, dtype=torch.int32, device=dev)
    edges_dev = torch.from_numpy(mass_edges(n_bins, z_range)).to(dev) if n_bins > 1 else None
    ws = torch.empty(M.dvae_mass_ws_doubles(n, dim, K, S, n_bins, sum_sizes), dtype=torch.float64, device=dev)
    mass = torch.empty(dim, n_bins * sum_sizes, dtype=torch.float64, device=dev)
    _masslib.call("dvae_mass_joint", ptr(table), ptr(logvar), ptr(rows), ptr(sizes_dev), ptr(edges_dev), n, dim, K, S, n_bins,
                  sum_sizes, ptr(ws), ptr(mass), _stream())
    scores = interpretability_scores_from_mass(mass.cpu().numpy(), lat_sizes, n_bins)     # ONE device->host copy
    scores.update(n_samples=S, n_bins=n_bins)
    return scores


# ---------------------------------------------------------------------- interventional robustness score on a table of means
def irs_group_map(lat_sizes, factor_bins=20):
    """The groups of step 1 of the IRS: -> (group_of_value int32 [sum(lat_sizes)], n_groups [K]).  factor_bins=None: every value of
    a factor is its own group; else value v of a factor with `size` values goes to bin numpy.digitize(v,
    numpy.histogram(numpy.arange(size), factor_bins)[1][:-1]) (disentanglement_lib's histogram discretiser; the edges come from the
    factor's full range 0 .. size - 1, not from a selection of rows), the distinct bins relabelled 0 .. G - 1 in order."""
    parts, n_groups = [], []
    for size in lat_sizes:
        values = np.arange(int(size))
        if factor_bins is not None:
            bins = np.digitize(values, np.histogram(values, int(factor_bins))[1][:-1])
            values = np.unique(bins, return_inverse=True)[1].reshape(-1)
        parts.append(values.astype(np.int32))
        n_groups.append(int(values.max()) + 1)
    return np.concatenate(parts), n_groups


def _check_irs_arguments(n, lat_sizes, diff_quantile, factor_bins, n_samples):
    _check_lat_sizes(lat_sizes, _irslib.MAX_FACTORS)
    if not 0.0 <= float(diff_quantile) <= 1.0:
        raise ValueError("diff_quantile must lie in [0, 1], got %r" % (diff_quantile,))
    if factor_bins is not None and int(factor_bins) < 1:
        raise ValueError("factor_bins must be >= 1 or None (every value its own group), got %r" % (factor_bins,))
    most = max(lat_sizes) if factor_bins is None else min(max(lat_sizes), int(factor_bins))
    if most > _irslib.MAX_GROUPS:
        raise ValueError("%d groups of one factor: the kernels take at most %d (use factor_bins)" % (most, _irslib.MAX_GROUPS))
    _check_n_samples(n, n_samples)


def irs_quantile_ranks(counts, diff_quantile):
    """numpy.percentile(x, 100 q) with the default linear method on n sorted values is a_lo + (a_hi - a_lo) t with
    h = (n - 1) (100 q / 100), lo = floor(h), hi = min(lo + 1, n - 1), t = h - lo.  -> (lo int64 [..] with -1 where n = 0, t)."""
    n = np.asarray(counts).astype(np.int64)
    h = (n - 1).clip(min=0) * (100.0 * float(diff_quantile) / 100.0)
    lo = np.floor(h)
    return np.where(n > 0, lo, -1).astype(np.int64), h - lo


def irs_from_statistics(counts, n_groups, stat_lo, stat_hi, dev_max, diff_quantile=0.99):
    """The host half of irs_from_table, fp64 (steps 4 to 6 of the score): counts int [total_groups], n_groups [K], and stat_lo,
    stat_hi, dev_max [total_groups, D] of dvae_irs_group_order_stats in its group index space (slot 0 = all selected rows, whose
    dev_max is the normaliser; the groups of factor k from 1 + sum(n_groups[:k])), stat_lo / stat_hi taken at the ranks of
    irs_quantile_ranks.

    max_diffs[g, d] = numpy.percentile's linear interpolation between the two order statistics; max_deviations[d] = dev_max[0, d];
    latent d is active iff max_deviations[d] > 0 and only active latents are scored (none: IRS = 0.0);
    IRS_matrix[a, k] = 1 - mean over the non-empty groups g of factor k of max_diffs[g, a] / max_deviations[a];
    disentanglement_scores[a] = max_k IRS_matrix[a, k], parents[a] the arg-max (the lowest k on ties); IRS = their average weighted
    by max_deviations.  Returns {"IRS", "disentanglement_scores" [A], "parents" [A], "IRS_matrix" [A, K] (the A active latents in
    order), "max_deviations" [D], "active" bool [D]}."""
    counts = np.asarray(counts).astype(np.int64).reshape(-1)
    n_groups = [int(g) for g in n_groups]
    lo, hi, mx = (np.asarray(a, dtype=np.float64) for a in (stat_lo, stat_hi, dev_max))
    total = 1 + sum(n_groups)
    assert counts.shape == (total,) and lo.shape == hi.shape == mx.shape and lo.shape[0] == total and lo.ndim == 2, (counts.shape, lo.shape)
    _rank, t = irs_quantile_ranks(counts, diff_quantile)
    t = t[:, None]
    diff = hi - lo
    max_diffs = np.where(t >= 0.5, hi - diff * (1.0 - t), lo + diff * t)                     # numpy's _lerp
    max_deviations = mx[0]
    active = max_deviations > 0
    K, A = len(n_groups), int(active.sum())
    matrix = np.zeros((A, K))
    start = 1
    for k, G in enumerate(n_groups):
        present = counts[start:start + G] > 0
        if A and present.any():
            matrix[:, k] = 1.0 - max_diffs[start:start + G][present][:, active].mean(axis=0) / max_deviations[active]
        start += G
    if A:
        scores, parents = matrix.max(axis=1), matrix.argmax(axis=1)
        irs = float(np.average(scores, weights=max_deviations[active]))
    else:
        scores, parents, irs = np.zeros(0), np.zeros(0, dtype=np.int64), 0.0
    return {"IRS": irs, "disentanglement_scores": scores, "parents": parents, "IRS_matrix": matrix,
            "max_deviations": max_deviations, "active": active}


def irs_from_table(mean, lat_sizes, diff_quantile=0.99, factor_bins=20, n_samples=None, seed=0, rows=None):
    """Interventional robustness score (Suter et al. 2019; disentanglement_lib's irs.py) of a representation given as the fp32
    [N, D] table ``mean`` (on the GPU) of a data set that enumerates ``lat_sizes`` in row-major order.

    For every group of selected rows that share a (binned, irs_group_map) factor value: the centre c = the mean of every latent
    (fp64 sums, rounded to fp32 once), the deviations |x - c| in fp32, and their diff_quantile-quantile as numpy.percentile
    interpolates it; the same over all selected rows gives the largest deviation per latent, the normaliser.  The rest is
    irs_from_statistics.  The groups' edges come from the full range of every factor: they are those of the selected rows'
    own values whenever the selection holds every factor's smallest and largest value; a group without a selected row does not
    exist for the score.

    n_samples=None: every row; else rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed
    gives the same bits, the global random states are untouched); ``rows`` ([S] row numbers in [0, N), repeats allowed) injects
    the selection.  Every size and argument is checked before any device work, and a table with a NaN or an infinity raises
    ValueError.  dvae_irs_group_means, ONE device-to-host copy of the counts, the ranks on the host, dvae_irs_group_order_stats
    with the device-resident means as centres, ONE copy of the statistics, the score in fp64 on the host.  Returns the dict of
    irs_from_statistics plus {"n_groups", "n_samples", "diff_quantile", "factor_bins"}: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K = len(lat_sizes)
    n, dim = _table_shape(mean)
    _check_irs_arguments(n, lat_sizes, diff_quantile, factor_bins, None if rows is not None else n_samples)
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if dim < 1:
        raise ValueError("mean must have one latent dimension or more")
    group_of_value, n_groups = irs_group_map(lat_sizes, factor_bins)
    total = 1 + sum(n_groups)
    if total * dim > _irslib.MAX_PAIRS:
        raise ValueError("%d groups x %d latents: the kernels take at most %d pairs" % (total, dim, _irslib.MAX_PAIRS))
    table, rows, S, dev = _select_rows(mean, rows, n_samples, seed, "irs_from_table", "interventional-robustness")
    R = _irslib.lib()
    st = _stream()
    sizes_dev = torch.tensor(lat_sizes, dtype=torch.int32, device=dev)
    map_dev = torch.from_numpy(group_of_value).to(dev)
    groups_dev = torch.tensor(n_groups, dtype=torch.int32, device=dev)
    layout = (n, dim, K, S, sum(lat_sizes), total, max(n_groups))
    ws = torch.empty(max(R.dvae_irs_group_means_ws_floats(n, dim, K, S, total),
                         R.dvae_irs_group_order_stats_ws_floats(n, dim, K, S, total), 1), dtype=torch.float32, device=dev)
    counts_dev = torch.empty(total, dtype=torch.int32, device=dev)
    means_dev = torch.empty(total, dim, dtype=torch.float32, device=dev)
    _irslib.call("dvae_irs_group_means", ptr(table), ptr(rows), ptr(sizes_dev), ptr(map_dev), ptr(groups_dev), *layout, ptr(ws),
                 ptr(counts_dev), ptr(means_dev), st)
    counts = counts_dev.cpu().numpy()                                                  # ONE device->host copy
    rank, _t = irs_quantile_ranks(counts, diff_quantile)
    rank[0] = S - 1                                                                    # all rows: only the largest deviation is used
    rank_dev = torch.from_numpy(rank.astype(np.int32)).to(dev)
    stats = torch.empty(3, total, dim, dtype=torch.float32, device=dev)
    _irslib.call("dvae_irs_group_order_stats", ptr(table), ptr(rows), ptr(sizes_dev), ptr(map_dev), ptr(groups_dev), ptr(means_dev),
                 ptr(rank_dev), *layout, ptr(ws), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), st)
    stat_lo, stat_hi, dev_max = stats.cpu().numpy()                                    # ONE copy of the statistics
    scores = irs_from_statistics(counts, n_groups, stat_lo, stat_hi, dev_max, diff_quantile)
    scores.update(n_groups=n_groups, n_samples=S, diff_quantile=float(diff_quantile),
                  factor_bins=None if factor_bins is None else int(factor_bins))
    return scores


# ---------------------------------------------------------------------- label-free scores on a table of means
def _check_unsupervised_arguments(n, dim, n_bins, n_samples):
    """n / dim: None where not known yet (a data set without __len__; before the encoder ran)."""
    if not 1 <= int(n_bins) <= _unsuplib.MAX_BINS:
        raise ValueError("n_bins must lie in [1, %d], got %r" % (_unsuplib.MAX_BINS, n_bins))
    if n_samples is not None and int(n_samples) < 1:
        raise ValueError("n_samples must be at least 1 or None, got %r" % (n_samples,))
    if n is not None:
        if n < 1:
            raise ValueError("the table of means must hold one row or more")
        _check_n_samples(n, n_samples)
    if dim is not None and not 1 <= dim <= _unsuplib.MAX_D:
        raise ValueError("mean must have between 1 and %d latent dimensions, got %d" % (_unsuplib.MAX_D, dim))


def unsupervised_scores_from_statistics(col_min, col_max, cov, counts, n_bins, active_threshold=0.01):
    """The host half of unsupervised_scores_from_table, fp64: col_min / col_max [D] and cov [D, D] of dvae_unsup_moments, ``counts``
    int [D (D - 1) / 2, n_bins, n_bins] of dvae_unsup_pair_hist (None or empty for D = 1).  disentanglement_lib's
    unsupervised_metrics.py on the posterior means:

    live [D] bool = col_max > col_min: an exactly constant column has variance 0, its logarithm would make every Gaussian score
    infinite, so it is dropped from them (as the IRS drops it);  C = cov on the live block, v = diag C;
    gaussian_total_correlation = KL(N(m, C) || N(m, diag v)) = 0.5 (sum log v - logdet C), inf when C is not positive definite to
    working precision (numpy.linalg.slogdet's sign), 0.0 with fewer than two live columns;
    gaussian_wasserstein_correlation = W2^2(N(m, C), N(m, diag v)) = 2 tr C - 2 tr sqrtm(diag(v) C) = 2 sum v - 2 sum sqrt(max(
    eigvalsh(V^1/2 C V^1/2), 0)) (the two matrices are similar; the symmetric form needs no scipy), and
    gaussian_wasserstein_correlation_norm = that / sum v; both 0.0 without a live column (eigvalsh leaves an ABSOLUTE error of about
    2^-53 max(v)^2 in every eigenvalue, so a live column whose variance is below 1e-4 of the largest costs the score up to
    1e-8 sum v: harmless for reading it, and the reason the tests keep their near-collapsed columns above that);
    mutual_information [D, D]: nats between the discretised columns d and e from the integer counts
    (mutual_information_from_counts), symmetric, zero diagonal;
    mutual_info_score = sum of it / (D^2 - D), over ALL D columns as disentanglement_lib does (0.0 for D = 1);
    active_units = #{d : cov[d, d] > active_threshold} (Burda et al. 2016);  variances = diag cov."""
    col_min, col_max = np.asarray(col_min), np.asarray(col_max)
    cov = np.asarray(cov, dtype=np.float64)
    D, n_bins = cov.shape[0], int(n_bins)
    assert cov.shape == (D, D) and col_min.shape == col_max.shape == (D,), (cov.shape, col_min.shape, col_max.shape)
    live = col_max > col_min
    C = cov[np.ix_(live, live)]
    v = np.diag(C).copy()
    tc = wass = wass_norm = 0.0
    if live.sum() >= 2:
        sign, logdet = np.linalg.slogdet(C)
        tc = float(0.5 * (np.log(v).sum() - logdet)) if sign > 0 else float("inf")
    if live.any():
        root = np.sqrt(v)
        eig = np.linalg.eigvalsh(root[:, None] * C * root[None, :])
        wass = float(2 * v.sum() - 2 * np.sqrt(np.maximum(eig, 0.0)).sum())
        wass_norm = float(wass / v.sum())
    mi = np.zeros((D, D))
    P = D * (D - 1) // 2
    if P:
        block = np.asarray(counts).astype(np.int64).reshape(P, n_bins, n_bins).astype(np.float64)
        upper = np.triu_indices(D, 1)                                    # (d, e), d < e, in lexicographic order: the pairs' own
        mi[upper] = mutual_information_from_counts(block)
        mi = mi + mi.T
    return {"gaussian_total_correlation": tc, "gaussian_wasserstein_correlation": wass,
            "gaussian_wasserstein_correlation_norm": wass_norm, "mutual_info_score": float(mi.sum() / (D * D - D)) if D > 1 else 0.0,
            "mutual_information": mi, "active_units": int((np.diag(cov) > active_threshold).sum()), "variances": np.diag(cov).copy(),
            "live": live}


def unsupervised_scores_from_table(mean, n_bins=20, n_samples=None, seed=0, rows=None, active_threshold=0.01):
    """Gaussian total correlation, Gaussian Wasserstein correlation and mean pairwise mutual information of a representation given as
    the fp32 [N, D] table ``mean`` (on the GPU), D <= 64 (formulas: unsupervised_scores_from_statistics).  No factor of variation is
    needed: this is what a data set without lat_sizes can be given.

    n_samples=None: every row; else rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed
    gives the same bits, the global random states are untouched); ``rows`` ([S] row numbers in [0, N), repeats allowed) injects
    the selection.  Every size and argument is checked before any device work, and a table with a NaN or an infinity raises
    ValueError.  dvae_unsup_moments, ONE device-to-host copy of its outputs (the covariance stays fp64 throughout), the bin edges
    of numpy.histogram on the host (histogram_edges: disentanglement_lib's histogram discretiser bit for bit),
    dvae_unsup_pair_hist (not for D = 1), ONE copy of the counts, the scores in fp64 on the host.  Returns the dict of
    unsupervised_scores_from_statistics plus {"n_samples", "n_bins"}: Python and numpy values."""
    n_bins = int(n_bins)
    n, dim = _table_shape(mean)
    _check_unsupervised_arguments(n, dim, n_bins, None if rows is not None else n_samples)
    table, rows, S, dev = _select_rows(mean, rows, n_samples, seed, "unsupervised_scores_from_table", "label-free score")
    U = _unsuplib.lib()
    st = _stream()
    ws = torch.empty(max(U.dvae_unsup_moments_ws_floats(n, dim, S), U.dvae_unsup_pair_hist_ws_floats(n, dim, S, n_bins), 1),
                     dtype=torch.float32, device=dev)
    out = torch.empty(dim * dim + 2 * dim, dtype=torch.float64, device=dev)      # cov, mean, then min and max: 2 D floats in D doubles
    cov_dev, mean_dev, minmax_dev = out[:dim * dim], out[dim * dim:dim * dim + dim], out[dim * dim + dim:].view(torch.float32)
    _unsuplib.call("dvae_unsup_moments", ptr(table), ptr(rows), n, dim, S, ptr(ws), ptr(minmax_dev[:dim]), ptr(minmax_dev[dim:]),
                   ptr(mean_dev), ptr(cov_dev), st)
    host = out.cpu()                                                               # ONE device->host copy
    cov = host[:dim * dim].numpy().reshape(dim, dim)
    minmax = host[dim * dim + dim:].view(torch.float32).numpy()
    col_min, col_max = minmax[:dim], minmax[dim:]
    counts = None
    if dim > 1:
        edges = np.stack([histogram_edges(col_min[d], col_max[d], n_bins) for d in range(dim)])
        edges_dev = torch.from_numpy(edges).to(dev)
        counts_dev = torch.empty(dim * (dim - 1) // 2, n_bins, n_bins, dtype=torch.int32, device=dev)
        _unsuplib.call("dvae_unsup_pair_hist", ptr(table), ptr(rows), ptr(edges_dev), n, dim, S, n_bins, ptr(ws), ptr(counts_dev), st)
        counts = counts_dev.cpu().numpy()                                          # ONE copy of the counts
    scores = unsupervised_scores_from_statistics(col_min, col_max, cov, counts, n_bins, active_threshold)
    scores.update(n_samples=S, n_bins=n_bins)
    return scores


# ---------------------------------------------------------------------- unsupervised disentanglement ranking on tables of q(z|x)
UDR_MAX_D = _unsuplib.MAX_D // 2                                         # a pair of models is one table of dvae_unsup_moments
UDR_CORRELATIONS = ("spearman", "lasso")
LASSO_STOP = 1e-13                                                       # largest coefficient change of a sweep
LASSO_MAX_SWEEPS = 100000


def _check_udr_arguments(n_models, n, dim, correlation="spearman", n_samples=None, seed=0, rows=None, kl_threshold=0.01,
                         filter_low_kl=True, lasso_alpha=0.1):
    """n / dim: None where not known yet (a data set without __len__; before the encoders ran).  The keyword arguments are those of
    udr_from_tables: an unknown one is a TypeError here, before any device work."""
    if n_models < 2:
        raise ValueError("UDR compares the models of a sweep: two or more are needed, got %d" % n_models)
    if correlation not in UDR_CORRELATIONS:
        raise ValueError("correlation must be one of %s, got %r" % (UDR_CORRELATIONS, correlation))
    if rows is None and n_samples is not None and int(n_samples) < 1:
        raise ValueError("n_samples must be at least 1 or None, got %r" % (n_samples,))
    if not (math.isfinite(float(kl_threshold)) and float(kl_threshold) >= 0):
        raise ValueError("kl_threshold must be a finite number >= 0, got %r" % (kl_threshold,))
    if not (math.isfinite(float(lasso_alpha)) and float(lasso_alpha) >= 0):
        raise ValueError("lasso_alpha must be a finite number >= 0, got %r" % (lasso_alpha,))
    int(seed)
    if n is not None:
        if n < 1:
            raise ValueError("the tables must hold one row or more")
        if rows is None:
            _check_n_samples(n, n_samples)
        if rows is None and (n if n_samples is None else int(n_samples)) > _udrlib.MAX_ROWS:
            raise ValueError("UDR ranks at most %d rows: pass n_samples" % _udrlib.MAX_ROWS)
    if dim is not None and not 1 <= dim <= UDR_MAX_D:
        raise ValueError("the tables must have between 1 and %d latent dimensions, got %d" % (UDR_MAX_D, dim))


def udr_pair_score(R):
    """disentanglement_lib's relative_strength_disentanglement of a non-negative [A, B] matrix, fp64:
    0.5 (mean_b max_a R^2 / sum_a R + mean_a max_b R^2 / sum_b R); a 0 / 0 term counts as 0; an EMPTY matrix (a model without an
    informative latent) scores 0.0 -- a stated deviation: disentanglement_lib raises there."""
    R = np.asarray(R, dtype=np.float64)
    if R.ndim != 2 or R.size == 0:
        return 0.0

    def side(axis):
        top, total = R.max(axis=axis) ** 2, R.sum(axis=axis)
        return float(np.mean(np.divide(top, total, out=np.zeros_like(top), where=total > 0)))
    return 0.5 * (side(0) + side(1))


def udr_model_scores(pairwise):
    """[M, M] pair scores -> [M]: the score of model i is the median over j != i of pairwise[j, i] (udr.py)."""
    pairwise = np.asarray(pairwise, dtype=np.float64)
    return np.array([np.median(np.delete(pairwise[:, i], i)) for i in range(pairwise.shape[0])])


def lasso_from_gram(G, c, alpha, stop=LASSO_STOP, max_sweeps=LASSO_MAX_SWEEPS):
    """argmin_w (1 / 2S) ||y - X w||^2 + alpha ||w||_1 from G = X^T X / S [A, A] and c = X^T y / S [A] by cyclic coordinate descent
    in fp64 (sklearn.linear_model.Lasso's objective and sweep order): w_a = soft(c_a - sum_{k != a} G_ak w_k, alpha) / G_aa; a
    coordinate with G_aa = 0 (a masked or constant latent) is skipped and stays 0; stops when the largest coefficient change of a
    sweep is <= ``stop``."""
    G, c = np.asarray(G, dtype=np.float64), np.asarray(c, dtype=np.float64)
    w = np.zeros(G.shape[0])
    live = [a for a in range(G.shape[0]) if G[a, a] > 0]
    for _sweep in range(max_sweeps):
        worst = 0.0
        for a in live:
            rho = c[a] - G[a] @ w + G[a, a] * w[a]
            new = math.copysign(max(abs(rho) - alpha, 0.0), rho) / G[a, a]
            worst = max(worst, abs(new - w[a]))
            w[a] = new
        if worst <= stop:
            break
    return w


def udr_correlation_from_cov(cov, mask_a, mask_b):
    """fp64 covariance [2D, 2D] of the concatenated tables of two models (a first) -> |Pearson correlation| block [D, D] of a's
    columns with b's, 0 where a variance is 0 or a latent is masked out."""
    D = cov.shape[0] // 2
    v = np.diag(cov)
    ok_a, ok_b = (v[:D] > 0) & mask_a, (v[D:] > 0) & mask_b
    R = np.zeros((D, D))
    blk = np.ix_(ok_a, ok_b)
    R[blk] = np.abs(cov[:D, D:][blk] / np.sqrt(np.outer(v[:D][ok_a], v[D:][ok_b])))
    return R


def udr_lasso_from_cov(cov, mask_a, mask_b, alpha):
    """fp64 covariance [2D, 2D] of the concatenated raw means of two models (a first) -> [D, D]: |w[a]| of latent a of model a when
    the Lasso predicts latent b of model b.  The Pearson blocks with zero-variance and masked columns as zero rows and columns ARE
    X^T X / S and X^T Y / S of disentanglement_lib's standardised, masked representations."""
    D = cov.shape[0] // 2
    v = np.diag(cov)
    ok = np.concatenate([(v[:D] > 0) & mask_a, (v[D:] > 0) & mask_b])
    corr = np.zeros_like(cov)
    blk = np.ix_(ok, ok)
    corr[blk] = cov[blk] / np.sqrt(np.outer(v[ok], v[ok]))
    G, C = corr[:D, :D], corr[:D, D:]
    return np.stack([np.abs(lasso_from_gram(G, C[:, b], alpha)) for b in range(D)], axis=1)


def udr_from_statistics(kl, cov_of_pair, correlation="spearman", kl_threshold=0.01, filter_low_kl=True, lasso_alpha=0.1):
    """The host half of udr_from_tables, fp64.  kl [M, D]: dvae_udr_kl_dims of every model; cov_of_pair(i, j), i < j: the [2D, 2D]
    covariance (dvae_unsup_moments) of model i's table beside model j's -- the rank tables for "spearman", the raw means for
    "lasso"."""
    kl = np.asarray(kl, dtype=np.float64)
    M, D = kl.shape
    mask = kl > kl_threshold
    raw, pairwise = np.zeros((M, M, D, D)), np.zeros((M, M))
    for i in range(M):
        for j in range(i + 1, M):
            cov = np.asarray(cov_of_pair(i, j), dtype=np.float64)
            flip = np.block([[cov[D:, D:], cov[D:, :D]], [cov[:D, D:], cov[:D, :D]]])
            if correlation == "spearman":
                raw[i, j] = udr_correlation_from_cov(cov, mask[i], mask[j])
                raw[j, i] = raw[i, j].T
            else:
                raw[i, j] = udr_lasso_from_cov(cov, mask[i], mask[j], lasso_alpha)
                raw[j, i] = udr_lasso_from_cov(flip, mask[j], mask[i], lasso_alpha)
            for a, b in ((i, j), (j, i)):
                pairwise[a, b] = udr_pair_score(raw[a, b][np.ix_(mask[a], mask[b])] if filter_low_kl else raw[a, b])
    return {"model_scores": udr_model_scores(pairwise), "pairwise_scores": pairwise, "raw_correlations": raw, "kl": kl,
            "n_active": mask.sum(axis=1)}


def udr_from_tables(means, logvars, correlation="spearman", n_samples=None, seed=0, rows=None, kl_threshold=0.01, filter_low_kl=True,
                    lasso_alpha=0.1):
    """Unsupervised disentanglement ranking (Duan et al. 2020; disentanglement_lib's udr.py) of M >= 2 models given as their fp32
    [N, D] tables of posterior means and log-variances (on the GPU; the same N and the same D <= 32 for all): no factor of
    variation is needed.

    kl [M, D] = dvae_udr_kl_dims of every model; a latent is informative when kl > kl_threshold.
    "spearman": dvae_udr_ranks of every model's means (exact tie-averaged ranks; ranks do not depend on standardisation, so none
    is applied), dvae_unsup_moments of the [S, 2D] rank tables of every pair, R_ij[a, b] = |cov / sqrt(var var)|, 0 where a
    variance is 0 or a latent is not informative.  "lasso": the same moments of the raw means; R_ij[a, b] = |w_a| of the Lasso
    (lasso_alpha; lasso_from_gram) that predicts latent b of model j from the latents of model i.
    pairwise_scores[i, j] = udr_pair_score of R_ij restricted to the informative latents (filter_low_kl), diagonal 0;
    model_scores[i] = the median over j != i of pairwise_scores[j, i].

    n_samples=None: every row; else rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed
    gives the same bits, the global random states are untouched); ``rows`` injects the selection; ONE selection serves every
    model.  Every size and argument is checked before any device work, and a table with a NaN or an infinity raises ValueError.
    All M models go through ONE dvae_unsup_moments call when M D <= 64.  Returns {"model_scores" [M], "pairwise_scores" [M, M],
    "raw_correlations" [M, M, D, D], "kl" [M, D], "n_active" [M], "n_samples", "correlation"}: Python and numpy values."""
    means, logvars = list(means), list(logvars)
    if len(means) != len(logvars):
        raise ValueError("means and logvars must hold one table per model, got %d and %d" % (len(means), len(logvars)))
    n, dim = _table_shape(means[0]) if means else (None, None)
    _check_udr_arguments(len(means), n, dim, correlation, n_samples, seed, rows, kl_threshold, filter_low_kl, lasso_alpha)
    for t in means + logvars:
        if _table_shape(t) != (n, dim):
            raise ValueError("every table must be [%d, %d] like the first, got %s" % (n, dim, tuple(t.shape)))
    if rows is not None:
        rows = _checked_rows(rows, n)
        if rows.numel() > _udrlib.MAX_ROWS:
            raise ValueError("UDR ranks at most %d rows" % _udrlib.MAX_ROWS)
    for name, tables in (("means", means), ("log-variances", logvars)):
        for t in tables:
            if not bool(torch.isfinite(t).all()):
                raise ValueError("a table of %s holds a NaN or an infinity" % name)
    M = len(means)
    first, rows, S, dev = _select_rows(means[0], rows, n_samples, seed, "udr_from_tables", "ranking")   # ONE selection for all models
    mus = [first] + [_select_rows(mu, rows, None, seed, "udr_from_tables", "ranking")[0] for mu in means[1:]]
    lvs = [lv.detach().to(device=dev, dtype=torch.float32).contiguous() for lv in logvars]
    L, U = _udrlib.lib(), _unsuplib.lib()
    st = _stream()
    one_call = M * dim <= _unsuplib.MAX_D
    wide = M * dim if one_call else 2 * dim
    ws = torch.empty(max(L.dvae_udr_ranks_ws_floats(n, dim, S), L.dvae_udr_kl_dims_ws_floats(n, dim, S),
                         U.dvae_unsup_moments_ws_floats(S if correlation == "spearman" else n, wide, S), 1),
                     dtype=torch.float32, device=dev)
    kl_dev = torch.empty(M, dim, dtype=torch.float64, device=dev)
    for i in range(M):
        _udrlib.call("dvae_udr_kl_dims", ptr(mus[i]), ptr(lvs[i]), ptr(rows), n, dim, S, ptr(ws), ptr(kl_dev[i]), st)
    if correlation == "spearman":                                                   # [S, D] rank tables: every row of them counts
        tabs = [torch.empty(S, dim, dtype=torch.float32, device=dev) for _ in range(M)]
        for i in range(M):
            _udrlib.call("dvae_udr_ranks", ptr(mus[i]), ptr(rows), n, dim, S, ptr(ws), ptr(tabs[i]), st)
        tab_rows, tab_n = None, S
    else:
        tabs, tab_rows, tab_n = mus, rows, n

    def moments(parts):
        both = torch.cat(parts, dim=1).contiguous()
        W = both.shape[1]
        out = torch.empty(W * W + 2 * W, dtype=torch.float64, device=dev)         # cov, mean, then min and max: 2 W floats in W doubles
        minmax = out[W * W + W:].view(torch.float32)
        _unsuplib.call("dvae_unsup_moments", ptr(both), ptr(tab_rows), tab_n, W, S, ptr(ws), ptr(minmax[:W]), ptr(minmax[W:]),
                       ptr(out[W * W:W * W + W]), ptr(out[:W * W]), st)
        return out[:W * W].cpu().numpy().reshape(W, W)
    if one_call:
        cov_all = moments(tabs)

        def cov_of_pair(i, j):
            at = np.concatenate([np.arange(i * dim, (i + 1) * dim), np.arange(j * dim, (j + 1) * dim)])
            return cov_all[np.ix_(at, at)]
    else:
        def cov_of_pair(i, j):
            return moments([tabs[i], tabs[j]])
    scores = udr_from_statistics(kl_dev.cpu().numpy(), cov_of_pair, correlation, kl_threshold, filter_low_kl, lasso_alpha)
    scores.update(n_samples=S, correlation=correlation)
    return scores


# ---------------------------------------------------------------------- DCI on a table of means
DCI_LEARNING_RATE = 0.1                                                  # GradientBoostingClassifier's default


def _check_dci_arguments(n, dim, lat_sizes, n_train=10000, n_test=5000, seed=0, rows=None, n_stages=100):
    """n: prod(lat_sizes); dim: None where not known yet (before the encoder ran)."""
    _check_lat_sizes(lat_sizes)
    if max(lat_sizes) > _dcilib.MAX_CLASSES:
        raise ValueError("a factor of variation with %d values: the boosted-tree kernels take at most %d classes"
                         % (max(lat_sizes), _dcilib.MAX_CLASSES))
    if not 1 <= int(n_train) <= _dcilib.MAX_ROWS:
        raise ValueError("n_train must lie in [1, %d], got %r" % (_dcilib.MAX_ROWS, n_train))
    if int(n_test) < 1:
        raise ValueError("n_test must be at least 1, got %r" % (n_test,))
    if not 1 <= int(n_stages) <= _dcilib.MAX_STAGES:
        raise ValueError("n_stages must lie in [1, %d], got %r" % (_dcilib.MAX_STAGES, n_stages))
    int(seed)
    if rows is None and int(n_train) + int(n_test) > n:
        raise ValueError("n_train + n_test must be at most %d (rows are drawn without replacement), got %d + %d"
                         % (n, int(n_train), int(n_test)))
    if dim is not None and not 1 <= dim <= _dcilib.MAX_D:
        raise ValueError("the table must have between 1 and %d latent dimensions, got %d" % (_dcilib.MAX_D, dim))


def dci_from_importance(importance):
    """disentanglement_lib's dci.py on the importance matrix [D, K] (latents x factors), fp64 -> (disentanglement, completeness):
    disentanglement = sum_d w_d (1 - H_K[(R_d. + 1e-11) normalised]), w_d = sum_k R_dk / sum R; completeness = sum_k w_k (1 -
    H_D[(R_.k + 1e-11) normalised]), w_k = sum_d R_dk / sum R; H_b the entropy to base b.  A matrix that sums to 0 weighs every
    latent and every factor alike (disentanglement_lib's fall-back), which gives 0 / 0; base 1 (one factor, one latent) has no
    entropy: that side counts as 1."""
    R = np.abs(np.asarray(importance, dtype=np.float64))
    if R.ndim != 2 or R.size == 0:
        raise ValueError("importance must be a non-empty [D, K] matrix, got shape %s" % (R.shape,))

    def one_minus_entropy(M, base):                                      # rows of M are distributions
        if base < 2:
            return np.ones(M.shape[0])
        P = (M + 1e-11) / (M + 1e-11).sum(axis=1, keepdims=True)
        return 1.0 + (P * np.log(P)).sum(axis=1) / math.log(base)
    D, K = R.shape
    per_code, per_factor = one_minus_entropy(R, K), one_minus_entropy(R.T, D)
    W = np.ones_like(R) if R.sum() == 0.0 else R
    return float((per_code * W.sum(axis=1) / W.sum()).sum()), float((per_factor * W.sum(axis=0) / W.sum()).sum())


def _factor_strides(lat_sizes):
    """stride_k of a data set that enumerates lat_sizes row-major: factor k of row r is (r // stride_k) % lat_sizes[k]."""
    return [int(np.prod(lat_sizes[k + 1:])) for k in range(len(lat_sizes))]


def _column_order(table, train):
    """int32 [D, S]: the stable ascending order of every column of table[train] -- dvae_dci_fit's `order`, ONE sort for all factors."""
    return torch.sort(table.index_select(0, train), dim=0, stable=True).indices.t().contiguous().to(torch.int32)


class _BoostedFactor:
    """The boosted-tree classifier of ONE factor of variation, fitted on the device: what dci_from_table and the prediction-based
    scores (downstream task, fairness) share.  The labels of the ``train`` rows are the ranks of the factor's values among those
    PRESENT in them (``classes``, sorted); dvae_dci_fit enqueues every stage; ``predict`` enqueues dvae_dci_predict on any row
    numbers of the table in calls of at most DVAE_DCI_MAX_ROWS rows and picks the class from the raw scores (two classes: the
    sign of the one score; more: the arg-max, the lowest class on ties).  One value present fits no tree and predicts that
    value; a row whose value was never seen counts as an error in ``accuracy``.  Nothing here is read back but the number of
    classes present (the size of the raw scores)."""

    def __init__(self, table, train, order, stride, size, n_stages, st):
        n, dim = int(table.shape[0]), int(table.shape[1])
        dev = table.device
        n_train = int(train.numel())
        self.table, self.stride, self.size, self.n_stages, self.st = table, int(stride), int(size), int(n_stages), st
        self.values_train = self.values_of(train)
        self.classes = torch.unique(self.values_train)                   # sorted; its length is the one number the host needs now
        self.C = C = int(self.classes.numel())
        self.T = T = _dcilib.trees(C)
        labels = torch.searchsorted(self.classes, self.values_train).to(torch.int32).contiguous()
        ws = torch.empty(max(_dcilib.lib().dvae_dci_fit_ws_floats(n, dim, n_train, C, n_stages), 2), dtype=torch.float32, device=dev)
        raw = torch.empty(n_train, T, dtype=torch.float64, device=dev)
        self.importance = torch.empty(dim, dtype=torch.float64, device=dev)
        self.n_split = torch.empty(1, dtype=torch.int32, device=dev)
        self.feature = torch.empty(n_stages, T, _dcilib.NODES, dtype=torch.int32, device=dev)
        self.stats = torch.empty(n_stages, T, _dcilib.NODES, _dcilib.NODE_STATS, dtype=torch.float64, device=dev)
        self.prior = torch.empty(T, dtype=torch.float64, device=dev)
        _dcilib.call("dvae_dci_fit", ptr(table), ptr(train), ptr(order), ptr(labels), n, dim, n_train, C, n_stages, DCI_LEARNING_RATE,
                     1, ptr(raw), ptr(self.prior), ptr(ws), ptr(self.importance), ptr(self.n_split), ptr(self.feature), ptr(self.stats),
                     st)
        self.picked_train = self._picked(raw)                            # the fit's own raw scores: the bits predict(train) gives

    def values_of(self, rows):
        """The factor's value of every row number."""
        return (rows // self.stride) % self.size

    def _picked(self, raw):
        return (raw[:, 0] > 0).long() if self.C == 2 else raw.argmax(dim=1)

    def predict(self, rows):
        """int64 [S]: the index into ``classes`` of the class predicted for table[rows] (rows int64 [S] on the device, each in
        [0, N): the kernel does not check them)."""
        n, dim = int(self.table.shape[0]), int(self.table.shape[1])
        rows = rows.contiguous()
        S = int(rows.numel())
        raw = self.prior.expand(S, self.T).contiguous()
        for lo in range(0, S, _dcilib.MAX_ROWS):
            part = min(_dcilib.MAX_ROWS, S - lo)
            _dcilib.call("dvae_dci_predict", ptr(self.table), ptr(rows[lo:lo + part]), n, dim, part, self.C, self.n_stages,
                         DCI_LEARNING_RATE, ptr(self.feature), ptr(self.stats), ptr(raw[lo:lo + part]), self.st)
        return self._picked(raw)

    def accuracy(self, picked, values):
        """fp64 scalar on the device: the share of rows whose predicted class is their value."""
        return (self.classes[picked] == values).double().mean()


def dci_from_table(mean, lat_sizes, n_train=10000, n_test=5000, seed=0, rows=None, n_stages=100):
    """DCI of a representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set that enumerates ``lat_sizes`` in
    row-major order: per factor a gradient-boosted classifier -- scikit-learn's GradientBoostingClassifier() restated
    (include/dvae_dci_hip.h), ``n_stages`` stages -- predicts the factor from the latents of n_train rows; its normalised
    feature importances are column k of the [D, K] importance matrix (dci_from_importance), its accuracy on the n_train rows and on
    n_test others is the informativeness.

    rows = randperm(N)[:n_train + n_test] from a private generator seeded with ``seed`` (the same seed gives the same bits, the
    global random states are untouched), the first n_train to fit; ``rows`` ([n_train + n_test] row numbers in [0, N), repeats
    allowed) injects the selection.  The factor values are digits of the row number; the labels of factor k are the ranks of its
    values among those PRESENT in the training rows (a test row with a value never seen counts as an error; a factor with one
    value present fits no tree: its column of the matrix is zero and its accuracy 1).  The columns are sorted ONCE (a stable
    torch.sort) for all factors; every stage of a factor is enqueued by ONE dvae_dci_fit call and nothing is read back until the
    importances and the predictions of all factors are there.  Every size and argument is checked before any device work, and
    a table with a NaN or an infinity raises ValueError.  Among exactly equal gains the lowest feature wins, where scikit-learn
    draws the order of the features from random_state.  Returns {"disentanglement", "completeness", "informativeness_train",
    "informativeness_test", "importance_matrix" [D, K], "n_train", "n_test", "n_stages"}: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_train, n_test, n_stages = len(lat_sizes), int(n_train), int(n_test), int(n_stages)
    n, dim = _table_shape(mean)
    _check_dci_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, n_test, seed, rows, n_stages)
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if rows is not None and torch.as_tensor(rows).numel() != n_train + n_test:
        raise ValueError("rows must hold n_train + n_test = %d row numbers" % (n_train + n_test))
    table, rows, _S, dev = _select_rows(mean, rows, n_train + n_test, seed, "dci_from_table", "boosted-tree")
    st = _stream()
    train, test = rows[:n_train].contiguous(), rows[n_train:].contiguous()
    order = _column_order(table, train)
    strides = _factor_strides(lat_sizes)
    fits = []
    for k in range(K):
        fit = _BoostedFactor(table, train, order, strides[k], lat_sizes[k], n_stages, st)
        fits.append((fit.importance, fit.n_split, fit.accuracy(fit.picked_train, fit.values_train),
                     fit.accuracy(fit.predict(test), fit.values_of(test))))
    matrix = np.zeros((dim, K))
    acc = np.zeros((K, 2))
    for k, (importance, n_split, acc_train, acc_test) in enumerate(fits):      # the read-back, after every factor was enqueued
        total, count = importance.cpu().numpy(), int(n_split.item())
        if count > 0 and total.sum() > 0:
            matrix[:, k] = np.abs(total / count / (total / count).sum())
        acc[k] = acc_train.item(), acc_test.item()
    disentanglement, completeness = dci_from_importance(matrix)
    return {"disentanglement": disentanglement, "completeness": completeness, "informativeness_train": float(acc[:, 0].mean()),
            "informativeness_test": float(acc[:, 1].mean()), "importance_matrix": matrix, "n_train": n_train, "n_test": n_test,
            "n_stages": n_stages}


# ---------------------------------------------------------------------- SAP with discrete factors on a table of means
def _check_sap_arguments(n, dim, lat_sizes, n_train=10000, n_test=5000, C=0.01, seed=0, rows=None):
    """n: prod(lat_sizes); dim: None where not known yet (before the encoder ran)."""
    _check_lat_sizes(lat_sizes, _saplib.MAX_FACTORS)
    if max(lat_sizes) > _saplib.MAX_CLASSES:
        raise ValueError("a factor of variation with %d values: the linear-SVM kernels take at most %d classes"
                         % (max(lat_sizes), _saplib.MAX_CLASSES))
    if not 1 <= int(n_train) <= _saplib.MAX_ROWS:
        raise ValueError("n_train must lie in [1, %d], got %r" % (_saplib.MAX_ROWS, n_train))
    if int(n_test) < 1:
        raise ValueError("n_test must be at least 1, got %r" % (n_test,))
    if not (isinstance(C, numbers.Real) and 0.0 < float(C) < math.inf):
        raise ValueError("C must be a positive finite number, got %r" % (C,))
    int(seed)
    if rows is None and int(n_train) + int(n_test) > n:
        raise ValueError("n_train + n_test must be at most %d (rows are drawn without replacement), got %d + %d"
                         % (n, int(n_train), int(n_test)))
    if dim is not None and not 1 <= dim <= _saplib.MAX_D:
        raise ValueError("the table must have between 1 and %d latent dimensions, got %d" % (_saplib.MAX_D, dim))


def sap_discrete_from_score_matrix(score_matrix):
    """disentanglement_lib's sap_score.py on its score matrix [D, K] (latents x factors; accuracies), fp64: the mean over the
    factors of the largest minus the second largest entry over the latents (largest_gap: one latent has no runner-up)."""
    m = np.asarray(score_matrix, dtype=np.float64)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("score_matrix must be a non-empty [D, K] matrix, got shape %s" % (m.shape,))
    return float(np.mean(largest_gap(m)))


def sap_discrete_from_table(mean, lat_sizes, n_train=10000, n_test=5000, C=0.01, seed=0, rows=None):
    """The SAP score with discrete factors of a representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set
    that enumerates ``lat_sizes`` in row-major order: score_matrix[d, k] is the accuracy on n_test rows of
    LinearSVC(C=C, class_weight="balanced") fitted on latent d ALONE to predict factor k from n_train rows -- the objective and
    its exact minimiser by Newton's method are stated in include/dvae_sap_hip.h, where liblinear stops at a tolerance.

    rows = randperm(N)[:n_train + n_test] from a private generator seeded with ``seed`` (the same seed gives the same bits, the
    global random states are untouched), the first n_train to fit; ``rows`` ([n_train + n_test] row numbers in [0, N), repeats
    allowed) injects the selection.  The factor values are digits of the row number; the labels of factor k are the ranks of its
    values among those PRESENT in the training rows (a test row with a value never seen counts as an error; a factor with one
    value present has no problem and predicts that value: every latent scores alike and its gap is 0).  Every problem of every
    (latent, factor) pair is fitted by ONE dvae_sap_fit call, and both dvae_sap_accuracy passes are enqueued, before anything is
    read back -- but the number of classes present per factor, which sizes ``coef``.  Every size and argument is checked before
    any device work, and a table with a NaN or an infinity raises ValueError.  Returns {"sap_discrete", "score_matrix" [D, K]
    (test accuracy), "score_matrix_train" [D, K], "coef" [D, P, 2] (w, b of every problem, include/dvae_sap_hip.h's order),
    "n_iterations_max", "n_train", "n_test", "C"}: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_train, n_test = len(lat_sizes), int(n_train), int(n_test)
    n, dim = _table_shape(mean)
    _check_sap_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, n_test, C, seed, rows)
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    if rows is not None and torch.as_tensor(rows).numel() != n_train + n_test:
        raise ValueError("rows must hold n_train + n_test = %d row numbers" % (n_train + n_test))
    table, rows, _S, dev = _select_rows(mean, rows, n_train + n_test, seed, "sap_discrete_from_table", "linear-SVM")
    st = _stream()
    train, test = rows[:n_train].contiguous(), rows[n_train:].contiguous()
    labels_train, labels_test, n_classes = [], [], []
    for stride, size in zip(_factor_strides(lat_sizes), lat_sizes):
        values_train, values_test = (train // stride) % size, (test // stride) % size
        classes = torch.unique(values_train)                             # sorted; its length is the one number the host needs now
        n_classes.append(int(classes.numel()))
        labels_train.append(torch.searchsorted(classes, values_train))
        at = torch.searchsorted(classes, values_test).clamp(max=n_classes[-1] - 1)
        labels_test.append(torch.where(classes[at] == values_test, at, torch.full_like(at, -1)))
    labels_train = torch.stack(labels_train).to(torch.int32).contiguous()
    labels_test = torch.stack(labels_test).to(torch.int32).contiguous()
    P = _saplib.problems(n_classes)
    host_classes = _saplib.host_classes(n_classes)
    coef = torch.empty(dim, P, 2, dtype=torch.float64, device=dev)
    iterations = torch.empty(dim, P, dtype=torch.int32, device=dev)
    correct = torch.empty(2, dim, K, dtype=torch.int32, device=dev)
    _saplib.call("dvae_sap_fit", ptr(table), ptr(train), ptr(labels_train), host_classes, n, dim, K, n_train, float(C), ptr(coef),
                 ptr(iterations), st)
    _saplib.call("dvae_sap_accuracy", ptr(table), ptr(train), ptr(labels_train), host_classes, n, dim, K, n_train, ptr(coef),
                 ptr(correct[0]), None, st)
    _saplib.call("dvae_sap_accuracy", ptr(table), ptr(test), ptr(labels_test), host_classes, n, dim, K, n_test, ptr(coef),
                 ptr(correct[1]), None, st)
    counts, steps, coef = correct.cpu().numpy(), iterations.cpu().numpy(), coef.cpu().numpy()      # the read-back
    if (steps < 1).any():
        raise _lib.DvaeHipError("dvae_sap_fit: %d of %d problems did not stop within %d Newton steps"
                                % (int((steps < 1).sum()), steps.size, _saplib.MAX_ITERATIONS))
    score_train, score_test = counts[0] / float(n_train), counts[1] / float(n_test)
    return {"sap_discrete": sap_discrete_from_score_matrix(score_test), "score_matrix": score_test, "score_matrix_train": score_train,
            "coef": coef, "n_iterations_max": int(steps.max()) if steps.size else 0, "n_train": n_train, "n_test": n_test,
            "C": float(C)}


# ---------------------------------------------------------------------- binning-free mutual information on a table of means
_EULER_GAMMA = "0.57721566490153286060651209008240243104215933593992"


def digamma_integers(n):
    """fp64 [n + 1]: psi(j) for j in [1, n] at index j (index 0 holds 0 and stands for nothing) -- the table dvae_knn_mi reads.
    The recurrence psi(1) = -gamma, psi(j + 1) = psi(j) + 1 / j carried in numpy's long double and rounded ONCE: a plain fp64
    cumulative sum is 31 ulp from scipy.special.digamma at n = 16 384, this is within 1 ulp (x86-64's 80-bit long double; where
    long double is fp64 it is the plain sum)."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1, got %r" % (n,))
    steps = np.concatenate([[-np.longdouble(_EULER_GAMMA)], np.longdouble(1) / np.arange(1, n, dtype=np.longdouble)])
    return np.concatenate([[0.0], np.cumsum(steps).astype(np.float64)])


def _check_knn_arguments(n, dim, lat_sizes, n_samples=10000, n_neighbors=3, seed=0, rows=None):
    """n: prod(lat_sizes); dim: None where not known yet (before the encoder ran)."""
    _check_lat_sizes(lat_sizes, _knnlib.MAX_FACTORS)
    if max(lat_sizes) > _knnlib.MAX_CLASSES:
        raise ValueError("a factor of variation with %d values: the k-NN mutual-information kernels take at most %d"
                         % (max(lat_sizes), _knnlib.MAX_CLASSES))
    if min(lat_sizes) < 2:
        raise ValueError("a factor of variation with one value has no entropy (the scores divide by it): lat_sizes=%s" % (lat_sizes,))
    if not (isinstance(n_neighbors, numbers.Integral) and 1 <= int(n_neighbors) <= _knnlib.MAX_NEIGHBORS):
        raise ValueError("n_neighbors must be an integer in [1, %d], got %r" % (_knnlib.MAX_NEIGHBORS, n_neighbors))
    int(seed)
    if rows is None:
        if n_samples is None:
            n_samples = n
        if not 1 <= int(n_samples) <= _knnlib.MAX_ROWS:
            raise ValueError("n_samples must lie in [1, %d] (a column is sorted in the LDS of one workgroup), got %r"
                             % (_knnlib.MAX_ROWS, n_samples))
        if int(n_samples) > n:
            raise ValueError("n_samples must be at most %d (rows are drawn without replacement), got %d" % (n, int(n_samples)))
    elif not 1 <= torch.as_tensor(rows).numel() <= _knnlib.MAX_ROWS:
        raise ValueError("rows must hold between 1 and %d row numbers, got %d" % (_knnlib.MAX_ROWS, torch.as_tensor(rows).numel()))
    if dim is not None and not 1 <= dim <= _knnlib.MAX_D:
        raise ValueError("the table must have between 1 and %d latent dimensions, got %d" % (_knnlib.MAX_D, dim))


def knn_information_scores_from_mi(mi, factor_entropy):
    """The host half of knn_information_scores_from_table, pure numpy, fp64: ``mi`` [D, K] the estimates of I(z_d; v_k) in nats
    (unclipped ones are clipped at 0 here and returned as ``raw``), ``factor_entropy`` [K] the entropy H_k in nats of factor k over
    all selected rows (a factor without entropy raises ValueError).  With I the clipped matrix and NMI = I / H_k:

    mig = mean_k (largest - second largest of I[:, k]) / H_k (one latent: the second is 0);  mig_sup = mean_d (largest - second
    largest over k of NMI[d, k]) (one factor: the second is 0; Li et al. 2020);  dcimig = sum_k max_{d : k(d) = k} gap_d / sum_k H_k,
    k(d) = arg max_k I[d, k], gap_d the largest minus the second largest of I[d, :] (a factor no latent prefers contributes 0;
    Sepliarskaia et al. 2019);  modularity = mean_d [1 - (sum m - t) / (t (K - 1))], m = I[d, :]^2, t = max m (0 where t = 0; K = 1:
    1 where t > 0; Ridgeway & Mozer 2018) -- the formulas of interpretability_scores_from_mass and
    information_scores_from_statistics on this matrix.
    A latent is ACTIVE if its row of I is not all zero, D_a of them.  InfoMEC (Hsu et al. 2023):
        infom = mean over the active d of (max_k NMI[d, k] / sum_k NMI[d, k] - 1 / K) / (1 - 1 / K)
        infoc = mean over the k with a nonzero column of (max_d NMI[d, k] / sum_d NMI[d, k] - 1 / D_a) / (1 - 1 / D_a)
    an entry whose denominator is 0 (K = 1, D_a = 1) is 1.0, and with no active latent both are 0.0.
    Returns {"mig", "mig_sup", "dcimig", "modularity", "infom", "infoc", "n_active", "best_latent" [K] (arg max_d, the lowest d on
    ties), "mutual_information" [D, K], "raw" [D, K], "factor_entropy" [K]}."""
    raw = np.array(mi, dtype=np.float64)
    H = np.array(factor_entropy, dtype=np.float64).reshape(-1)
    if raw.ndim != 2 or raw.size == 0 or H.shape != (raw.shape[1],) or not np.isfinite(raw).all():
        raise ValueError("mi must be a finite non-empty [D, K] matrix and factor_entropy [K], got shapes %s and %s" % (raw.shape, H.shape))
    if not (H > 0).all():
        raise ValueError("factor(s) %s take one value among the selected rows: no entropy to divide the scores by"
                         % [k for k in range(len(H)) if not H[k] > 0])
    I = np.maximum(raw, 0.0)
    D, K = I.shape
    nmi = I / H[None, :]
    m = I ** 2
    t = m.max(axis=1)
    modularity_d = np.zeros(D)
    if K > 1:
        modularity_d[t > 0] = 1.0 - (m.sum(axis=1) - t)[t > 0] / (t[t > 0] * (K - 1))
    else:
        modularity_d[t > 0] = 1.0
    mig_sup_d = largest_gap(nmi.T)
    gap_d = largest_gap(I.T)
    prefers = I.argmax(axis=1)                                           # [D], k(d)
    dcimig = sum(gap_d[prefers == k].max() for k in range(K) if (prefers == k).any()) / H.sum()
    active = (I != 0).any(axis=1)
    n_active = int(active.sum())
    infom = infoc = 0.0
    if n_active:
        A = nmi[active]
        infom = 1.0 if K == 1 else float(np.mean((A.max(axis=1) / A.sum(axis=1) - 1.0 / K) / (1.0 - 1.0 / K)))
        A = A[:, (A != 0).any(axis=0)]
        infoc = 1.0 if n_active == 1 else float(np.mean((A.max(axis=0) / A.sum(axis=0) - 1.0 / n_active) / (1.0 - 1.0 / n_active)))
    return {"mig": float(np.mean(largest_gap(I) / H)), "mig_sup": float(mig_sup_d.mean()), "dcimig": float(dcimig),
            "modularity": float(modularity_d.mean()), "infom": infom, "infoc": infoc, "n_active": n_active,
            "best_latent": I.argmax(axis=0).astype(np.int64), "mutual_information": I, "raw": raw, "factor_entropy": H}


def knn_information_scores_from_table(mean, lat_sizes, n_samples=10000, n_neighbors=3, seed=0, rows=None):
    """Binning-free MIG, modularity, MIG-sup, DCIMIG, InfoM and InfoC of a representation given as the fp32 [N, D] table ``mean``
    (on the GPU) of a data set that enumerates ``lat_sizes`` in row-major order (formulas: knn_information_scores_from_mi).
    I(z_d; v_k) is the k-nearest-neighbour estimate between a continuous and a discrete variable (Ross 2014) that
    include/dvae_knn_hip.h states: scikit-learn's _compute_mi_cd on the column as it is -- mutual_info_classif's rescaling and
    seeded noise are NOT applied, ties are handled by the estimator's own rule.

    rows = randperm(N)[:n_samples] from a private generator seeded with ``seed`` (the same seed gives the same bits, the global
    random states are untouched; n_samples=None: every row); ``rows`` ([S] row numbers in [0, N), repeats allowed: a repeated row
    counts as another row) injects the selection.  At most DVAE_KNN_MAX_ROWS rows: a column is sorted in the LDS of one workgroup.
    The factor values are digits of the row number; a factor with one value among the selected rows raises ValueError.  Every
    size and argument is checked before any device work, and a table with a NaN or an infinity raises ValueError.  ONE launch
    sequence (dvae_knn_sort, dvae_knn_mi), ONE device-to-host copy of the sums and the class counts, the clipping at 0 and
    everything after it in fp64 on the host.  Returns the dictionary of knn_information_scores_from_mi and "n_kept" [D, K] (the rows
    whose class has another row), "n_samples", "n_neighbors": Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K = len(lat_sizes)
    n, dim = _table_shape(mean)
    _check_knn_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_samples, n_neighbors, seed, rows)
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))
    table, rows, S, dev = _select_rows(mean, rows, n_samples, seed, "knn_information_scores_from_table", "k-NN mutual-information")
    Kn = _knnlib.lib()
    st = _stream()
    sum_sizes = sum(lat_sizes)
    host_sizes = _knnlib.host_sizes(lat_sizes)
    psi = digamma_integers(S)
    psi_dev = torch.from_numpy(psi).to(dev)
    ws = torch.empty(max(Kn.dvae_knn_ws_bytes(n, dim, S), 8), dtype=torch.uint8, device=dev)
    out = torch.empty(4 * dim * K + (K * sum_sizes + 1) // 2, dtype=torch.float64, device=dev)     # the sums, then the int32 counts
    sums, counts = out[:4 * dim * K], out[4 * dim * K:].view(torch.int32)[:K * sum_sizes]
    _knnlib.call("dvae_knn_sort", ptr(table), ptr(rows), n, dim, S, ptr(ws), st)
    _knnlib.call("dvae_knn_mi", ptr(rows), host_sizes, n, dim, K, S, int(n_neighbors), ptr(psi_dev), ptr(ws), ptr(sums), ptr(counts),
                 None, None, st)
    host = out.cpu()                                                     # ONE device->host copy
    sums = host[:4 * dim * K].numpy().reshape(dim, K, 4)
    counts = host[4 * dim * K:].view(torch.int32)[:K * sum_sizes].numpy().reshape(K, sum_sizes)
    H, start = np.zeros(K), 0
    for k, size in enumerate(lat_sizes):
        pv = counts[k, start:start + size].astype(np.float64) / S
        H[k] = -(pv[pv > 0] * np.log(pv[pv > 0])).sum()
        start += size
    n_kept = np.rint(sums[:, :, 0]).astype(np.int64)
    kept = np.maximum(n_kept, 1)
    raw = np.where(n_kept > 0, psi[kept] + sums[:, :, 1] / kept - sums[:, :, 2] / kept - sums[:, :, 3] / kept, 0.0)
    scores = knn_information_scores_from_mi(raw, H)
    scores.update(n_kept=n_kept, n_samples=S, n_neighbors=int(n_neighbors))
    return scores


# ---------------------------------------------------------------------- prediction-based scores on a table of means
def _check_table_enumerates(n, lat_sizes):
    if n != int(np.prod(lat_sizes)):
        raise ValueError("data set of %d images does not enumerate lat_sizes=%s" % (n, lat_sizes))


def _prediction_table(mean, caller, kernels):
    """_select_rows without a selection: the table must be finite, then on the GPU -> (table fp32 contiguous, device)."""
    table, _rows, _S, dev = _select_rows(mean, None, None, 0, caller, kernels)
    return table, dev


def _check_downstream_arguments(n, dim, lat_sizes, n_train=(10, 100, 1000, 10000), n_test=5000, seed=0, rows=None, n_stages=100):
    """n: prod(lat_sizes); dim: None where not known yet.  Every size of n_train is held to _check_dci_arguments, in the order given."""
    try:
        sizes = [int(s) for s in n_train]
    except TypeError:
        raise ValueError("n_train must be a sequence of training-set sizes, got %r" % (n_train,)) from None
    if not sizes or len(set(sizes)) != len(sizes):
        raise ValueError("n_train must hold one size or more, each once, got %r" % (n_train,))
    if rows is not None and len(rows) != len(sizes):
        raise ValueError("rows must hold one selection per size of n_train: %d, got %d" % (len(sizes), len(rows)))
    for i, size in enumerate(sizes):
        _check_dci_arguments(n, dim, lat_sizes, size, n_test, seed, None if rows is None else rows[i], n_stages)
    return sizes


def downstream_task_aggregates(sizes, acc_train, acc_test):
    """The result of downstream_task_from_table from the accuracies [len(sizes), K] (fp64) of every size and factor: per size n the
    mean and the smallest accuracy over the factors and every factor's own, and for every n below the largest
    "{n}:efficiency" = mean test accuracy at n / mean test accuracy at the largest n (disentanglement_lib's downstream_task.py;
    0 / 0 counts as 0)."""
    acc_train, acc_test = np.asarray(acc_train, dtype=np.float64), np.asarray(acc_test, dtype=np.float64)
    out = {}
    for i, n in enumerate(sizes):
        for name, acc in (("train", acc_train[i]), ("test", acc_test[i])):
            out["%d:mean_%s_accuracy" % (n, name)] = float(acc.mean())
            out["%d:min_%s_accuracy" % (n, name)] = float(acc.min())
            for k, a in enumerate(acc):
                out["%d:%s_accuracy_factor_%d" % (n, name, k)] = float(a)
    largest = max(sizes)
    top = out["%d:mean_test_accuracy" % largest]
    for n in sizes:
        if n != largest:
            out["%d:efficiency" % n] = out["%d:mean_test_accuracy" % n] / top if top > 0 else 0.0
    return out


def downstream_task_from_table(mean, lat_sizes, n_train=(10, 100, 1000, 10000), n_test=5000, seed=0, rows=None, n_stages=100):
    """Downstream-task score (Locatello et al. 2019, section 5.4; disentanglement_lib's downstream_task.py with its
    gradient-boosting predictor) of a representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set that
    enumerates ``lat_sizes`` in row-major order: for every training-set size n of ``n_train``, in the order given, the boosted-tree
    classifier of dci_from_table (_BoostedFactor: libdvae_dci_hip.so) is fitted per factor on n rows and its accuracy is taken
    on those rows and on n_test others -- the launches of dci_from_table(n_train=n, rows=rows_n), whose informativeness_train /
    informativeness_test are "{n}:mean_train_accuracy" / "{n}:mean_test_accuracy" here, bit for bit.

    rows_n = randperm(N)[:n + n_test], one draw per size from ONE private generator seeded with ``seed`` (the same seed gives the
    same bits, the global random states are untouched), the first n to fit; ``rows`` (a list with one [n + n_test] selection per
    size, row numbers in [0, N), repeats allowed) injects them.  Labels, unseen values and a factor with one value present: as in
    dci_from_table.  Every size and argument is checked before any device work (the limits are dci_from_table's, per size), a
    table with a NaN or an infinity raises ValueError, and nothing is read back until every fit and prediction of every size is
    enqueued.  Returns downstream_task_aggregates' keys plus "n_train" (the list), "n_test", "n_stages": Python values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_test, n_stages = len(lat_sizes), int(n_test), int(n_stages)
    n, dim = _table_shape(mean)
    sizes = _check_downstream_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, n_test, seed, rows, n_stages)
    _check_table_enumerates(n, lat_sizes)
    if rows is not None:
        for size, r in zip(sizes, rows):
            if torch.as_tensor(r).numel() != size + n_test:
                raise ValueError("rows must hold n_train + n_test = %d row numbers for n_train = %d" % (size + n_test, size))
        rows = [_checked_rows(r, n) for r in rows]
    table, dev = _prediction_table(mean, "downstream_task_from_table", "boosted-tree")
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    st = _stream()
    strides = _factor_strides(lat_sizes)
    enqueued = []
    for i, size in enumerate(sizes):
        if rows is not None:
            rows_n = rows[i].to(dev).contiguous()
        else:
            rows_n = torch.randperm(n, generator=gen, device=dev)[:size + n_test].contiguous()
        train, test = rows_n[:size].contiguous(), rows_n[size:].contiguous()
        order = _column_order(table, train)
        for k in range(K):
            fit = _BoostedFactor(table, train, order, strides[k], lat_sizes[k], n_stages, st)
            enqueued.append(torch.stack([fit.accuracy(fit.picked_train, fit.values_train),
                                         fit.accuracy(fit.predict(test), fit.values_of(test))]))
    acc = torch.stack(enqueued).cpu().numpy().reshape(len(sizes), K, 2)            # ONE read-back, after everything was enqueued
    scores = downstream_task_aggregates(sizes, acc[:, :, 0], acc[:, :, 1])
    scores.update(n_train=sizes, n_test=n_test, n_stages=n_stages)
    return scores


def intervened_rows(base, stride, size):
    """Row numbers [size, P] of the rows ``base`` [P] (a tensor of row numbers of a data set that enumerates its factors
    row-major) after an intervention on the factor with this stride and size: row c has that factor set to c and every other
    factor as in ``base`` -- base - ((base // stride) % size) * stride + c * stride."""
    cleared = base - ((base // stride) % size) * stride
    return cleared.unsqueeze(0) + torch.arange(size, dtype=base.dtype, device=base.device).unsqueeze(1) * stride


def unfairness_from_counts(counts):
    """disentanglement_lib's inter_group_fairness of a count matrix [classes predicted, values of the sensitive factor], fp64:
    overall = counts.sum(1) / counts.sum(), p_c = counts[:, c] / counts[:, c].sum(), tv_c = 0.5 sum_y |p_c[y] - overall[y]| ->
    (sum_c tv_c n_c / sum_c n_c, max_c tv_c) with n_c the column sums; a column without a row takes no part."""
    counts = np.asarray(counts, dtype=np.float64)
    if counts.ndim != 2 or counts.size == 0 or counts.sum() <= 0:
        raise ValueError("counts must be a [classes, values] matrix that counts one row or more, got shape %s" % (counts.shape,))
    n_c = counts.sum(axis=0)
    overall = counts.sum(axis=1) / counts.sum()
    live = np.flatnonzero(n_c > 0)
    tv = np.array([0.5 * np.abs(counts[:, c] / n_c[c] - overall).sum() for c in live])      # a column at a time: one order of summation
    return float((tv * n_c[live]).sum() / n_c[live].sum()), float(tv.max())


def fairness_from_counts(counts, K):
    """The host half of fairness_from_table, fp64.  counts: {(i, j): the count matrix of target i under interventions on j}, every
    ordered pair of the K >= 2 factors -> the two [K, K] matrices of unfairness_from_counts (diagonal 0), their means over the
    off-diagonal entries and the means of the rows / columns of the first without the diagonal entry."""
    mean_m, max_m = np.zeros((K, K)), np.zeros((K, K))
    for (i, j), c in counts.items():
        mean_m[i, j], max_m[i, j] = unfairness_from_counts(c)
    off = ~np.eye(K, dtype=bool)
    return {"mean_unfairness_matrix": mean_m, "max_unfairness_matrix": max_m, "mean_unfairness": float(mean_m[off].mean()),
            "max_unfairness": float(max_m[off].mean()), "mean_unfairness_per_target": mean_m.sum(axis=1) / (K - 1),
            "mean_unfairness_per_sensitive": mean_m.sum(axis=0) / (K - 1)}


def _check_fairness_arguments(n, dim, lat_sizes, n_train=10000, n_test_per_value=100, seed=0, n_stages=100, rows=None, base_rows=None):
    """n: prod(lat_sizes); dim: None where not known yet.  The limits of _check_dci_arguments; the base rows are drawn WITH
    replacement, so only n_train is held to the size of the data set."""
    _check_dci_arguments(n, dim, lat_sizes, n_train, 1, seed, (), n_stages)       # (): the sum n_train + n_test is not this score's
    if len(lat_sizes) < 2:
        raise ValueError("fairness needs a target and a sensitive factor: two factors of variation or more, got lat_sizes=%s" % (lat_sizes,))
    if int(n_test_per_value) < 1:
        raise ValueError("n_test_per_value must be at least 1, got %r" % (n_test_per_value,))
    if rows is None and int(n_train) > n:
        raise ValueError("n_train must be at most %d (rows are drawn without replacement), got %d" % (n, int(n_train)))


def fairness_from_table(mean, lat_sizes, n_train=10000, n_test_per_value=100, seed=0, n_stages=100, rows=None, base_rows=None,
                        return_details=False):
    """Unfairness of a representation (Locatello et al. 2019b, On the Fairness of Disentangled Representations;
    disentanglement_lib's fairness.py) given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set that enumerates
    ``lat_sizes`` in row-major order: how much the prediction of a target factor i moves when a sensitive factor j is intervened
    on.  Per factor i the boosted-tree classifier of dci_from_table (_BoostedFactor: libdvae_dci_hip.so) is fitted ONCE on
    n_train rows; for every ordered pair (i, j), j != i, in row-major order, P = n_test_per_value base rows are drawn uniformly
    WITH replacement, factor j of every base row is set to each of its values c in turn (intervened_rows: row arithmetic, no copy
    of the table) and all size_j P rows are predicted on the device (dvae_dci_predict, at most DVAE_DCI_MAX_ROWS rows a call);
    counts[y, c] = the rows of column c predicted as class y (a bincount on the device; y runs over the classes present in the
    training rows); mean_unfairness[i, j], max_unfairness[i, j] = unfairness_from_counts(counts), in fp64 on the host.

    Training rows = randperm(N)[:n_train], then the base rows = randint(N, [P]) pair by pair, from ONE private generator seeded
    with ``seed`` (the same seed gives the same bits, the global random states are untouched); ``rows`` ([n_train] row numbers
    in [0, N), repeats allowed) and ``base_rows`` ([K, K, P], the diagonal is not used) inject them, each on its own.  Every size
    and argument is checked before any device work, a table with a NaN or an infinity raises ValueError, and nothing is read
    back until every fit and prediction is enqueued.  Returns {"mean_unfairness_matrix", "max_unfairness_matrix" [K, K] (target
    x sensitive, diagonal 0), "mean_unfairness", "max_unfairness" (the means of the two matrices over their off-diagonal
    entries, as disentanglement_lib reports them), "mean_unfairness_per_target", "mean_unfairness_per_sensitive" [K] (the means of
    a row / a column of the first matrix without its diagonal entry), "n_train", "n_test_per_value", "n_stages"}: Python and numpy
    values.  return_details=True: (scores, details) with "classes" (per factor the values present in training) and "predicted"
    ({(i, j): the predicted VALUES of factor i, int64 [size_j, P]}), host copies."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_train, P, n_stages = len(lat_sizes), int(n_train), int(n_test_per_value), int(n_stages)
    n, dim = _table_shape(mean)
    _check_fairness_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, P, seed, n_stages, rows, base_rows)
    _check_table_enumerates(n, lat_sizes)
    if rows is not None:
        if torch.as_tensor(rows).numel() != n_train:
            raise ValueError("rows must hold n_train = %d row numbers" % n_train)
        rows = _checked_rows(rows, n)
    if base_rows is not None:
        base_rows = torch.as_tensor(base_rows).to(torch.int64)
        if tuple(base_rows.shape) != (K, K, P) or not (0 <= int(base_rows.min()) and int(base_rows.max()) < n):
            raise ValueError("base_rows must have shape (%d, %d, %d) and hold row numbers in [0, %d)" % (K, K, P, n))
    table, dev = _prediction_table(mean, "fairness_from_table", "boosted-tree")
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    st = _stream()
    strides = _factor_strides(lat_sizes)
    train = rows.to(dev).contiguous() if rows is not None else torch.randperm(n, generator=gen, device=dev)[:n_train].contiguous()
    if base_rows is not None:
        base_rows = base_rows.to(dev)
    order = _column_order(table, train)
    fits = [_BoostedFactor(table, train, order, strides[k], lat_sizes[k], n_stages, st) for k in range(K)]
    counted, predicted = {}, {}
    for i in range(K):
        for j in range(K):
            if j == i:
                continue
            base = base_rows[i, j] if base_rows is not None else torch.randint(n, (P,), generator=gen, device=dev)
            picked = fits[i].predict(intervened_rows(base, strides[j], lat_sizes[j]).reshape(-1))       # [size_j * P], column c first
            column = torch.arange(lat_sizes[j], device=dev).repeat_interleave(P)
            counted[i, j] = torch.bincount(picked * lat_sizes[j] + column, minlength=fits[i].C * lat_sizes[j])
            if return_details:
                predicted[i, j] = fits[i].classes[picked].view(lat_sizes[j], P)
    # the read-back, after everything was enqueued
    scores = fairness_from_counts({(i, j): c.cpu().numpy().reshape(fits[i].C, lat_sizes[j]) for (i, j), c in counted.items()}, K)
    scores.update(n_train=n_train, n_test_per_value=P, n_stages=n_stages)
    if not return_details:
        return scores
    return scores, {"classes": [f.classes.cpu() for f in fits], "predicted": {ij: v.cpu() for ij, v in predicted.items()}}


def auc_from_rank_sums(rank_sum, n_pos, n_rows):
    """One-vs-rest ROC AUC of every class from the sum R+ of the tie-averaged ranks (1-based, among all n_rows scores of the class's
    column) of its n+ positive rows: (R+ - n+ (n+ + 1) / 2) / (n+ n-), the Mann-Whitney form, fp64 -> (auc [C], NaN for a class
    without positives or without negatives; the mean over the other classes, NaN when there is none)."""
    rank_sum, n_pos = np.asarray(rank_sum, dtype=np.float64), np.asarray(n_pos, dtype=np.float64)
    n_neg = float(n_rows) - n_pos
    ok = (n_pos > 0) & (n_neg > 0)
    auc = np.full(rank_sum.shape, np.nan)
    auc[ok] = (rank_sum[ok] - n_pos[ok] * (n_pos[ok] + 1.0) / 2.0) / (n_pos[ok] * n_neg[ok])
    return auc, (float(np.mean(auc[ok])) if ok.any() else float("nan"))


def explicitness_from_aucs(auc_train, auc_test):
    """The per-factor AUCs [K] (NaN: a factor without a class that has positives and negatives) -> the result of
    explicitness_from_table without its sizes: the means over the factors that have an AUC, NaN when there is none."""
    out = {}
    for name, a in (("train", np.asarray(auc_train, dtype=np.float64)), ("test", np.asarray(auc_test, dtype=np.float64))):
        have = ~np.isnan(a)
        out["explicitness_" + name] = float(np.mean(a[have])) if have.any() else float("nan")
        out["explicitness_%s_per_factor" % name] = a
    return out


def class_probabilities(W, b, features):
    """softmax(features W^T + b) in fp64 on the CPU, [n, C]."""
    return torch.softmax(torch.as_tensor(features, dtype=torch.float64) @ W.t() + b, dim=1)


def explicitness_from_table(mean, lat_sizes, n_train=10000, n_test=5000, seed=0, rows=None, return_details=False, fit="host"):
    """Explicitness (Ridgeway & Mozer 2018; the second half of disentanglement_lib's modularity_explicitness.py) of a
    representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set that enumerates ``lat_sizes`` in row-major
    order: per factor the multinomial logistic regression of the beta-VAE score (fit_logistic_regression, C = 1.0, fp64 on the
    CPU) predicts the factor from the raw latents of n_train rows -- labels are the ranks of the factor's values among those
    PRESENT in the training rows --; its class probabilities of the training and of the test rows are rounded to fp32 and every
    class column is ranked on the device (dvae_udr_ranks of libdvae_udr_hip.so: exact tie-averaged ranks, at most DVAE_UDR_MAX_D
    columns a call); the one-vs-rest AUC of a class is the rank sum of its rows (auc_from_rank_sums, summed in fp64: the ranks
    are half-integers, the sum is exact), the AUC of a factor the mean over its classes with both positives and negatives among
    the evaluated rows.  scikit-learn's roc_auc_score raises for a class without positives; here that class is left out, a factor
    without any such class (one value present: no negatives among the training rows) is NaN in the per-factor arrays and left
    out of the means (NaN when no factor is left).  A test row with a value never seen in training is a negative of every class.

    Rows as in dci_from_table: randperm(N)[:n_train + n_test] from a private generator seeded with ``seed``, the first n_train to
    fit; ``rows`` injects the selection.  Every size and argument is checked before any device work (the limits of
    dci_from_table) and a table with a NaN or an infinity raises ValueError.  Returns {"explicitness_train", "explicitness_test",
    "explicitness_train_per_factor", "explicitness_test_per_factor" [K], "n_train", "n_test"}: Python and numpy values.
    return_details=True: (scores, details) with per factor "classes", "W", "b", the fp32 "probabilities_train" /
    "probabilities_test" that were ranked, "labels_train" / "labels_test" (-1: a value never seen) and the per-class AUCs.
    fit="device": the K regressions are fitted by ONE dvae_lr_fit call on the gathered rows where they lie (libdvae_lr_hip.so: the
    same objective to tolerance_grad 1e-8; a fit that does not get there raises DvaeHipError) and the probabilities come from
    dvae_lr_predict (formed in fp64, rounded once) without leaving the device; at most 8 factors and 64 latents then."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_train, n_test = len(lat_sizes), int(n_train), int(n_test)
    n, dim = _table_shape(mean)
    _check_dci_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, n_test, seed, rows, 1)
    _check_fit(fit, n_train, dim, lat_sizes)
    _check_table_enumerates(n, lat_sizes)
    if rows is not None and torch.as_tensor(rows).numel() != n_train + n_test:
        raise ValueError("rows must hold n_train + n_test = %d row numbers" % (n_train + n_test))
    table, rows, _S, dev = _select_rows(mean, rows, n_train + n_test, seed, "explicitness_from_table", "ranking")
    L = _udrlib.lib()
    st = _stream()
    strides = _factor_strides(lat_sizes)
    sets = (("train", slice(0, n_train)), ("test", slice(n_train, n_train + n_test)))
    if fit == "device":
        probes = _DeviceProbes(table, rows, n_train, lat_sizes, 1.0, LR_TOLERANCE_GRAD, False, st, with_prob=True)
        on_device = probes.per_factor("explicitness_from_table")         # the read-back of the coefficients and of the solver's report
    else:
        features = table.index_select(0, rows).cpu().double()                      # [n_train + n_test, D]: the fit is the host's
    rows_host = rows.cpu()
    enqueued, details = [], []
    for k in range(K):
        values = (rows_host // strides[k]) % lat_sizes[k]
        classes = torch.unique(values[:n_train])                         # sorted
        C = int(classes.numel())
        at = torch.searchsorted(classes, values).clamp(max=C - 1)
        labels = torch.where(classes[at] == values, at, torch.full_like(at, -1))   # -1: a value never seen in training
        if fit == "device":
            W, b = on_device[k]["W"], on_device[k]["b"]
        elif C > 1:
            W, b = fit_logistic_regression(features[:n_train], labels[:n_train], C, C=1.0)
        else:                                                            # one class: nothing to fit
            W, b = torch.zeros(1, dim, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        detail = {"classes": classes, "W": W, "b": b}
        for name, part in sets:
            S = part.stop - part.start
            if fit == "device":
                prob = on_device[k]["prob_" + name]                      # [S, C] fp32, where dvae_lr_predict wrote it
            else:
                prob = class_probabilities(W, b, features[part]).to(torch.float32).to(dev)               # [S, C], rounded to fp32
            lab = labels[part].to(dev)
            rank_sum = torch.empty(C, dtype=torch.float64, device=dev)
            for lo in range(0, C, _udrlib.MAX_D):
                cols = prob[:, lo:lo + _udrlib.MAX_D].contiguous()
                width = int(cols.shape[1])
                ws = torch.empty(max(L.dvae_udr_ranks_ws_floats(S, width, S), 1), dtype=torch.float32, device=dev)
                ranks = torch.empty(S, width, dtype=torch.float32, device=dev)
                _udrlib.call("dvae_udr_ranks", ptr(cols), None, S, width, S, ptr(ws), ptr(ranks), st)
                own = lab.unsqueeze(1) == torch.arange(lo, lo + width, device=dev).unsqueeze(0)
                rank_sum[lo:lo + width] = (ranks.double() * own).sum(dim=0)
            n_pos = torch.bincount(lab + 1, minlength=C + 1)[1:]
            enqueued.append((k, name, S, rank_sum, n_pos))
            detail["probabilities_" + name], detail["labels_" + name] = prob, labels[part]
        details.append(detail)
    per_factor = {"train": np.full(K, np.nan), "test": np.full(K, np.nan)}
    for k, name, S, rank_sum, n_pos in enqueued:                                   # the read-back, after every ranking was enqueued
        auc, per_factor[name][k] = auc_from_rank_sums(rank_sum.cpu().numpy(), n_pos.cpu().numpy(), S)
        details[k]["auc_" + name] = auc
    scores = explicitness_from_aucs(per_factor["train"], per_factor["test"])
    scores.update(n_train=n_train, n_test=n_test)
    if not return_details:
        return scores
    for d in details:
        d["probabilities_train"], d["probabilities_test"] = d["probabilities_train"].cpu(), d["probabilities_test"].cpu()
    return scores, details


# ---------------------------------------------------------------------- linear-softmax probes fitted on the device
LR_TOLERANCE_GRAD = 1e-8                                                 # fit_logistic_regression's own


def _check_lr_sizes(n_rows, dim, n_classes):
    """The limits of libdvae_lr_hip.so, before any device work.  dim: None where not known yet."""
    n_classes = [int(c) for c in n_classes]
    if not 1 <= len(n_classes) <= _lrlib.MAX_PROBLEMS:
        raise ValueError("%d problems of one call: the softmax-regression kernels take between 1 and %d" % (len(n_classes), _lrlib.MAX_PROBLEMS))
    if not all(1 <= c <= _lrlib.MAX_CLASSES for c in n_classes):
        raise ValueError("a problem with %d classes: the softmax-regression kernels take between 1 and %d"
                         % (max(n_classes) if min(n_classes) >= 1 else min(n_classes), _lrlib.MAX_CLASSES))
    if not 1 <= int(n_rows) <= _lrlib.MAX_ROWS:
        raise ValueError("the softmax-regression kernels fit between 1 and %d rows, got %r" % (_lrlib.MAX_ROWS, n_rows))
    if dim is not None and not 1 <= int(dim) <= _lrlib.MAX_D:
        raise ValueError("the softmax-regression kernels take between 1 and %d features, got %d" % (_lrlib.MAX_D, dim))


def _check_lr_numbers(C, tolerance_grad):
    if not (isinstance(C, numbers.Real) and 0.0 < float(C) < math.inf):
        raise ValueError("C must be a positive finite number, got %r" % (C,))
    if not (isinstance(tolerance_grad, numbers.Real) and 0.0 <= float(tolerance_grad) < math.inf):
        raise ValueError("tolerance_grad must be a finite number >= 0, got %r" % (tolerance_grad,))


def _check_fit(fit, n_train, dim, lat_sizes):
    """fit = "host" | "device" of the scores that fit a logistic regression; "device" is held to libdvae_lr_hip.so's limits."""
    if fit not in ("host", "device"):
        raise ValueError('fit must be "host" or "device", got %r' % (fit,))
    if fit == "device":
        _check_lr_sizes(n_train, dim, lat_sizes)


def _standardizer_on_the_device(features, st):
    """(shift, scale) fp64 [D] on the device of the fp32 [S, D] features: the column mean and 1 / population std from
    dvae_unsup_moments (fp64 throughout); a constant column -- its largest element is its smallest -- gets scale 0."""
    S, D = int(features.shape[0]), int(features.shape[1])
    dev = features.device
    ws = torch.empty(max(_unsuplib.lib().dvae_unsup_moments_ws_floats(S, D, S), 1), dtype=torch.float32, device=dev)
    out = torch.empty(D * D + 2 * D, dtype=torch.float64, device=dev)     # cov, mean, then min and max: 2 D floats in D doubles
    minmax = out[D * D + D:].view(torch.float32)
    _unsuplib.call("dvae_unsup_moments", ptr(features), None, S, D, S, ptr(ws), ptr(minmax[:D]), ptr(minmax[D:]), ptr(out[D * D:D * D + D]),
                   ptr(out[:D * D]), st)
    var = out[:D * D].view(D, D).diagonal() * ((S - 1.0) / S)             # ddof = 1 -> the population variance
    live = (minmax[D:] > minmax[:D]) & (var > 0)
    scale = torch.where(live, torch.rsqrt(torch.where(live, var, torch.ones_like(var))), torch.zeros_like(var))
    return out[D * D:D * D + D].contiguous(), scale.contiguous()


def _lr_fit(features, labels, n_classes, C, tolerance_grad, shift, scale, st):
    """dvae_lr_fit enqueued: features fp32 [S, D], labels int32 [Q, S], both contiguous on the device -> (coef fp64 flat, report
    fp64 [Q, 4]) on the device.  Nothing is read back."""
    S, D, Q = int(features.shape[0]), int(features.shape[1]), len(n_classes)
    dev = features.device
    host = _lrlib.host_classes(n_classes)
    n_bytes = _lrlib.lib().dvae_lr_ws_bytes(S, D, host, Q)
    if n_bytes < 0:
        raise ValueError("dvae_lr_ws_bytes refuses S = %d, D = %d, classes %s" % (S, D, list(n_classes)))
    ws = torch.empty(max(n_bytes // 8, 1), dtype=torch.float64, device=dev)
    coef = torch.empty(sum(_lrlib.coef_sizes(n_classes, D)), dtype=torch.float64, device=dev)
    report = torch.empty(Q, 4, dtype=torch.float64, device=dev)
    _lrlib.call("dvae_lr_fit", ptr(features), ptr(shift), ptr(scale), ptr(labels), host, S, D, Q, float(C), float(tolerance_grad), ptr(ws),
                ptr(coef), ptr(report), st)
    return coef, report


def _lr_predict(features, labels, n_classes, coef, shift, scale, st, with_prob):
    """dvae_lr_predict enqueued -> {"prob": fp32 flat or None, "log_loss" fp64 [Q], "correct", "counted" int32 [Q]} on the device."""
    T, D, Q = int(features.shape[0]), int(features.shape[1]), len(n_classes)
    dev = features.device
    out = {"prob": torch.empty(T * sum(n_classes), dtype=torch.float32, device=dev) if with_prob else None,
           "log_loss": torch.empty(Q, dtype=torch.float64, device=dev), "correct": torch.empty(Q, dtype=torch.int32, device=dev),
           "counted": torch.empty(Q, dtype=torch.int32, device=dev)}
    _lrlib.call("dvae_lr_predict", ptr(features), ptr(shift), ptr(scale), ptr(labels), _lrlib.host_classes(n_classes), T, D, Q, ptr(coef),
                ptr(out["prob"]), ptr(out["log_loss"]), ptr(out["correct"]), ptr(out["counted"]), st)
    return out


def _lr_converged(report, caller):
    """The host copy of the solver's report [Q, 4]; DvaeHipError naming the first problem that stopped short of tolerance_grad."""
    report = report.cpu().numpy()
    short = np.flatnonzero(report[:, 2] < 0)
    if short.size:
        q = int(short[0])
        raise _lib.DvaeHipError("%s: dvae_lr_fit: problem %d (of %d; %d in all) did not meet tolerance_grad within %d Newton steps: max |gradient| "
                                "%.3e after %d function evaluations" % (caller, q, report.shape[0], short.size, _lrlib.MAX_ITERATIONS,
                                                                        report[q, 1], int(report[q, 3])))
    return report


def _split_coef(coef, n_classes, dim):
    """The flat host coefficients -> [(W [C, D], b [C])] fp64 tensors, one per problem."""
    out, at = [], 0
    for C in n_classes:
        out.append((coef[at:at + C * dim].view(C, dim).clone(), coef[at + C * dim:at + C * (dim + 1)].clone()))
        at += C * (dim + 1)
    return out


def fit_logistic_regression_device(features, labels, n_classes, C=1.0, tolerance_grad=LR_TOLERANCE_GRAD, standardize=False,
                                   return_report=False):
    """fit_logistic_regression's problem -- minimise mean cross-entropy + ||W||^2 / (2 C n) with an unpenalised bias, from zero --
    solved ON THE DEVICE by dvae_lr_fit (libdvae_lr_hip.so: truncated Newton-CG in fp64, one launch) until the largest absolute
    gradient entry is at most ``tolerance_grad``.  features [n, D] (n <= 16384, D <= 64) on the GPU, rounded to fp32 if they are not;
    labels [n] in [0, n_classes), n_classes <= 256.  Returns (W [n_classes, D], b [n_classes]) as fp64 CPU tensors like the host
    function, b on sum b = 0; unlike it, a fit that stops short of the tolerance raises DvaeHipError naming the problem.
    standardize=True fits on (x - column mean) / population std (a constant column: on 0) and returns the coefficients folded back to
    the raw features (W scale, b - W scale . shift).  return_report=True: (W, b, report) with the solver's (objective, max |gradient|,
    Newton steps, function evaluations)."""
    features = torch.as_tensor(features)
    if features.dim() != 2:
        raise ValueError("features must be an [n, D] matrix, got shape %s" % (tuple(features.shape),))
    n, dim = int(features.shape[0]), int(features.shape[1])
    _check_lr_sizes(n, dim, [n_classes])
    _check_lr_numbers(C, tolerance_grad)
    labels = torch.as_tensor(labels).reshape(-1)
    if labels.numel() != n or not (0 <= int(labels.min()) and int(labels.max()) < int(n_classes)):
        raise ValueError("labels must hold %d classes in [0, %d)" % (n, int(n_classes)))
    if not bool(torch.isfinite(features).all()):
        raise ValueError("the features hold a NaN or an infinity")
    if not features.is_cuda:
        raise _lib.DvaeHipError("fit_logistic_regression_device needs the features on the GPU (there is no CPU / PyTorch fallback for the "
                                "softmax-regression kernels)")
    dev = features.device
    x = features.detach().to(torch.float32).contiguous()
    y = labels.to(dev, torch.int32).view(1, n).contiguous()
    st = _stream()
    shift, scale = _standardizer_on_the_device(x, st) if standardize else (None, None)
    coef, report = _lr_fit(x, y, [int(n_classes)], C, tolerance_grad, shift, scale, st)
    report = _lr_converged(report, "fit_logistic_regression_device")
    W, b = _split_coef(coef.cpu(), [int(n_classes)], dim)[0]
    if standardize:
        shift, scale = shift.cpu(), scale.cpu()
        W = W * scale
        b = b - W @ shift
    return (W, b, report[0]) if return_report else (W, b)


class _DeviceProbes:
    """The linear-softmax probes of every factor of variation, fitted and evaluated on the device: what explicitness_from_table
    (fit="device") and infoe_from_table share.  rows int64 [n_train + n_test] on the device, the first n_train to fit; the labels of
    factor k are the ranks of its values among those PRESENT in the training rows (-1 for a test row whose value is not).  ONE
    dvae_lr_fit call fits all K problems on the gathered rows and two dvae_lr_predict calls evaluate them; nothing is read back here
    but the number of classes present per factor, which sizes the coefficients."""

    def __init__(self, table, rows, n_train, lat_sizes, C, tolerance_grad, standardize, st, with_prob):
        self.dim, self.n_train, self.n_test = int(table.shape[1]), int(n_train), int(rows.numel()) - int(n_train)
        gathered = table.index_select(0, rows)                           # the torch gather is plumbing
        self.x = {"train": gathered[:n_train].contiguous(), "test": gathered[n_train:].contiguous()}
        train, test = rows[:n_train], rows[n_train:]
        labels_train, labels_test, self.n_classes, self.classes = [], [], [], []
        for stride, size in zip(_factor_strides(lat_sizes), lat_sizes):
            values_train, values_test = (train // stride) % size, (test // stride) % size
            classes = torch.unique(values_train)                         # sorted; its length is the one number the host needs now
            self.n_classes.append(int(classes.numel()))
            self.classes.append(classes)
            labels_train.append(torch.searchsorted(classes, values_train))
            at = torch.searchsorted(classes, values_test).clamp(max=self.n_classes[-1] - 1)
            labels_test.append(torch.where(classes[at] == values_test, at, torch.full_like(at, -1)))
        self.labels = {"train": torch.stack(labels_train).to(torch.int32).contiguous(),
                       "test": torch.stack(labels_test).to(torch.int32).contiguous()}
        self.shift, self.scale = _standardizer_on_the_device(self.x["train"], st) if standardize else (None, None)
        self.coef, self.report = _lr_fit(self.x["train"], self.labels["train"], self.n_classes, C, tolerance_grad, self.shift, self.scale, st)
        self.out = {name: _lr_predict(self.x[name], self.labels[name], self.n_classes, self.coef, self.shift, self.scale, st, with_prob)
                    for name in ("train", "test") if self.x[name].shape[0] > 0}

    def per_factor(self, caller):
        """The read-back of the report (raises where a fit stopped short) and of the coefficients -> per factor {"W", "b" (fp64, CPU),
        "prob_train", "prob_test" (fp32 [rows, C] views on the device, where the probabilities were asked for)}."""
        self.report_host = _lr_converged(self.report, caller)
        out = [{"W": W, "b": b} for W, b in _split_coef(self.coef.cpu(), self.n_classes, self.dim)]
        for name, got in self.out.items():
            at, rows = 0, int(self.x[name].shape[0])
            for k, C in enumerate(self.n_classes):
                if got["prob"] is not None:
                    out[k]["prob_" + name] = got["prob"][at:at + rows * C].view(rows, C)
                at += rows * C
        return out


def _beta_vae_on_the_device(feats, labels, factor_vae_train, factor_vae_eval, active, n_train, n_eval, L, st, return_details, details):
    """The beta-VAE half of factor_scores_from_table with fit="device": feats fp32 [V, D] and labels int32 [V] of the train and the
    eval set where dvae_score_pair_absdiff left them; the classes are the factors that occur in the train set."""
    dim = int(feats["train"].shape[1])
    factor = {k: v.to(torch.int64) for k, v in labels.items()}
    classes = torch.unique(factor["train"])                              # sorted; its length sizes the coefficients
    C = int(classes.numel())
    ranks = {}
    for key in ("train", "eval"):
        at = torch.searchsorted(classes, factor[key]).clamp(max=C - 1)
        ranks[key] = torch.where(classes[at] == factor[key], at, torch.full_like(at, -1)).to(torch.int32).view(1, -1).contiguous()
    coef, report = _lr_fit(feats["train"], ranks["train"], [C], 1.0, LR_TOLERANCE_GRAD, None, None, st)
    counts = {key: _lr_predict(feats[key], ranks[key], [C], coef, None, None, st, False)["correct"] for key in ("train", "eval")}
    _lr_converged(report, "factor_scores_from_table")
    scores = {"factor_vae_train": factor_vae_train, "factor_vae_eval": factor_vae_eval,
              "beta_vae_train": int(counts["train"].item()) / float(n_train), "beta_vae_eval": int(counts["eval"].item()) / float(n_eval),
              "n_active": int(active.sum()), "n_train": n_train, "n_eval": n_eval, "batch_size": L}
    if not return_details:
        return scores
    W, b = _split_coef(coef.cpu(), [C], dim)[0]
    details.update(features_train=feats["train"].cpu().double(), features_eval=feats["eval"].cpu().double(),
                   labels_train=factor["train"].cpu(), labels_eval=factor["eval"].cpu(), classes=classes.cpu(), W=W, b=b)
    return scores, details


# ---------------------------------------------------------------------- InfoE on a table of means
def _check_infoe_arguments(n, dim, lat_sizes, n_train=10000, n_test=5000, C=1.0, seed=0, rows=None):
    """n: prod(lat_sizes); dim: None where not known yet.  The rows and checks of explicitness_from_table / dci_from_table, then the
    limits of libdvae_lr_hip.so."""
    _check_dci_arguments(n, dim, lat_sizes, n_train, n_test, seed, rows, 1)
    _check_lr_sizes(n_train, dim, lat_sizes)
    _check_lr_numbers(C, 0.0)


def infoe_from_log_loss(ce_model, ce_null):
    """The InfoE of Hsu et al. 2023 (the normalised predictive V-information of a factor given the latents, V = linear-softmax
    probes) from two cross-entropies per factor, pure numpy: ce_model [K], the mean negative log-likelihood of the probe, and
    ce_null [K], that of the best constant prediction (the class frequencies of the training rows: their entropy on those rows).
    -> (per_factor [K] = 1 - ce_model / ce_null, UNCLIPPED, NaN where ce_null is not positive -- a factor with one class present --
    or a cross-entropy is not finite; the mean over the other factors of max(0, .), NaN when there is none)."""
    ce_model, ce_null = np.asarray(ce_model, dtype=np.float64), np.asarray(ce_null, dtype=np.float64)
    if ce_model.shape != ce_null.shape or ce_model.ndim != 1:
        raise ValueError("ce_model and ce_null must be two [K] vectors, got shapes %s and %s" % (ce_model.shape, ce_null.shape))
    ok = np.isfinite(ce_model) & np.isfinite(ce_null)
    ok[ok] = ce_null[ok] > 0
    per_factor = np.full(ce_model.shape, np.nan)
    per_factor[ok] = 1.0 - ce_model[ok] / ce_null[ok]
    return per_factor, (float(np.maximum(per_factor[ok], 0.0).mean()) if ok.any() else float("nan"))


def infoe_from_table(mean, lat_sizes, n_train=10000, n_test=5000, C=1.0, standardize=True, seed=0, rows=None):
    """InfoE -- explicitness in the InfoMEC triple of Hsu et al. 2023, next to InfoM and InfoC of knn_information_scores_from_table --
    of a representation given as the fp32 [N, D] table ``mean`` (on the GPU) of a data set that enumerates ``lat_sizes`` in row-major
    order: per factor k the multinomial logistic regression of include/dvae_lr_hip.h (fit_logistic_regression's objective with this
    ``C``) predicts the factor from all latents of n_train rows; with ce_model = its mean negative log-likelihood and ce_null = the
    cross-entropy of the class frequencies OF THE TRAINING ROWS (on them: the empirical entropy H(s_k)),
    infoe_per_factor = 1 - ce_model / ce_null (infoe_from_log_loss), on the training rows and on n_test others.  theta = (0, log
    frequencies) is feasible at no penalty, so the training value is >= 0 up to the solver's tolerance.

    Rows and checks as in explicitness_from_table / dci_from_table: randperm(N)[:n_train + n_test] from a private generator seeded
    with ``seed`` (the same seed gives the same bits, the global random states are untouched), the first n_train to fit; ``rows``
    injects the selection.  Labels are the ranks of the values PRESENT in the training rows; a test row whose value was never seen
    is left out of ce_model_test and ce_null_test (n_unseen counts them) and is an error in accuracy_test.  standardize=True fits on
    (x - shift) scale with shift = the column mean and scale = 1 / population std of the training rows (dvae_unsup_moments, fp64; a
    constant column gets scale 0 and weights exactly 0).  All K factors are fitted by ONE dvae_lr_fit call and evaluated by two
    dvae_lr_predict calls before anything is read back but the number of classes present per factor; a fit that stops short of
    tolerance_grad = 1e-8 raises DvaeHipError.  At most 8 factors, 256 values a factor, 64 latents, 10 240 training rows.
    Returns {"infoe_train", "infoe_test" (the means over the factors with two classes or more of max(0, .)),
    "infoe_train_per_factor", "infoe_test_per_factor" [K] (unclipped; NaN for a one-class factor), "ce_model_train", "ce_model_test",
    "ce_null_train", "ce_null_test", "accuracy_train", "accuracy_test" [K], "n_unseen" [K], "report" [K, 4] (the solver's objective,
    max |gradient|, Newton steps, function evaluations), "n_train", "n_test", "C", "standardize"}: Python and numpy values."""
    lat_sizes = [int(k) for k in lat_sizes]
    K, n_train, n_test = len(lat_sizes), int(n_train), int(n_test)
    n, dim = _table_shape(mean)
    _check_infoe_arguments(int(np.prod(lat_sizes)) if lat_sizes else 0, dim, lat_sizes, n_train, n_test, C, seed, rows)
    _check_table_enumerates(n, lat_sizes)
    if rows is not None and torch.as_tensor(rows).numel() != n_train + n_test:
        raise ValueError("rows must hold n_train + n_test = %d row numbers" % (n_train + n_test))
    table, rows, _S, dev = _select_rows(mean, rows, n_train + n_test, seed, "infoe_from_table", "softmax-regression")
    st = _stream()
    probes = _DeviceProbes(table, rows, n_train, lat_sizes, float(C), LR_TOLERANCE_GRAD, bool(standardize), st, with_prob=False)
    width = max(probes.n_classes)
    counts = torch.stack([torch.stack([torch.bincount(probes.labels[name][k] + 1, minlength=width + 1)[1:] for k in range(K)])
                          for name in ("train", "test")])                # [2, K, width] rows per class (the unseen ones left out)
    # ---- the read-back, after everything was enqueued
    report = _lr_converged(probes.report, "infoe_from_table")
    counts = counts.cpu().numpy().astype(np.float64)
    got = {name: {k: v.cpu().numpy() for k, v in out.items() if v is not None} for name, out in probes.out.items()}
    result = {}
    for i, (name, total) in enumerate((("train", n_train), ("test", n_test))):
        counted = got[name]["counted"].astype(np.float64)
        freq = counts[0] / float(n_train)                                # the class frequencies of the TRAINING rows
        with np.errstate(divide="ignore", invalid="ignore"):
            log_freq = np.where(counts[0] > 0, np.log(np.where(counts[0] > 0, freq, 1.0)), 0.0)
            ce_null = -(counts[i] * log_freq).sum(axis=1) / counted
            ce_model = got[name]["log_loss"] / counted
        per_factor, score = infoe_from_log_loss(ce_model, ce_null)
        result.update({"infoe_" + name: score, "infoe_%s_per_factor" % name: per_factor, "ce_model_" + name: ce_model,
                       "ce_null_" + name: ce_null, "accuracy_" + name: got[name]["correct"] / float(total)})
    result.update(n_unseen=(n_test - got["test"]["counted"]).astype(np.int64), report=report, n_train=n_train, n_test=n_test, C=float(C),
                  standardize=bool(standardize))
    return result

"""dags_vae_search_amd — MI355X-native DAG-VAE (PACE) train-step hot path of rlog58/dags-vae-search.

Drop-in surface for that path: PaceVaeV3, train_batch, pace_collate_fn, collate_graph_batch, load_model_state,
LabeledDag (row codec).  Structure learning next to it, on three kinds of data: BNLearnWrapper (discrete), GaussianEvaluator
(real-valued) and MixedEvaluator (factors and real columns) under hill_climb and tabu_search.  latent_bo_search: Bayesian optimisation of the BIC in the VAE's latent space.  evaluate_reconstruction: model_test with
the isomorphism judging on the device.  All arithmetic runs in libdvs_hip.so (hand-written HIP for gfx950); there is no CPU path.
"""
from .features import LabeledDag, LabeledGraph, collate_graph_batch, pace_collate_fn, prepare_features  # noqa: F401
from .pace import PaceVaeV3  # noqa: F401
from .train import batch_test, load_model_state, model_test, train_batch, train_model  # noqa: F401
from . import optim  # noqa: F401
from .records import CompactBatch, CompactDagDataset, encode_graphs  # noqa: F401
from .bic import AvailableCaseEvaluator, BNLearnWrapper  # noqa: F401
from .evaluator import Evaluator  # noqa: F401
from .predictor_data import create_predictor_dataset, generate_predictor_graphs_batch, prepare_predictor_data  # noqa: F401
from .datasets import LabeledDagDatasetInMemory, LabeledDagDatasetInMemoryTest  # noqa: F401
from .search import (SearchResult, StructureSet, decoded_structures, generation_metrics, latent_bo_search,  # noqa: F401
                     optimize_acquisition)
from .recon import evaluate_reconstruction, match_decoded  # noqa: F401
from .generate import DagStream, create_encoder_dataset, encoder_dag_train_schema, generate_dags  # noqa: F401
from .hillclimb import HillClimbResult, decode_move, hill_climb  # noqa: F401
from .tabu import TabuResult, tabu_search  # noqa: F401
from .compare import StructureComparison, compare_structures, cpdag, equivalence_classes, shd  # noqa: F401
from .exact import ExactResult, exact_from_tables, exact_search, local_score_table  # noqa: F401
from .pc import PCResult, ci_test, ci_tests, pc_stable, skeleton_blacklist  # noqa: F401
from .local import MMPCResult, RSMAX2Result, ci_tests_group, mmhc, mmpc, rsmax2  # noqa: F401
from .params import FittedBN, bn_fit, cross_validate, cv_folds, log_likelihood, sample  # noqa: F401
# posterior.py is imported before infer.py: loading a submodule binds its name in the package, and the name `posterior` must end
# up as infer.posterior, the function it has always been (the module stays reachable as dags_vae_search_amd.posterior in
# sys.modules and through `from dags_vae_search_amd.posterior import ...`)
from .posterior import ArcPosterior, arc_posterior, arc_posterior_from_tables  # noqa: F401
# ordermc.py is named after no function it exports, so it needs no such care
from .ordermc import FamilyScores, OrderMCMCResult, family_scores, order_mcmc  # noqa: F401
from .infer import cpdist, cpquery, posterior, predict  # noqa: F401
from .eliminate import (EliminationPlan, elimination_plan, evidence_probability, exact_cpquery, exact_joint,  # noqa: F401
                        exact_posterior)
from .incomplete import (EMResult, ExpectedCounts, StructuralEMResult, available_case_evaluator, em_fit,  # noqa: F401
                         expected_counts, family_plans, fit_counts, impute, incomplete_rows, structural_em, target_plans)
from .mixed import (FittedCGBN, MixedEvaluator, cg_cross_validate, cg_fit, cg_log_likelihood, cg_predict,  # noqa: F401
                    cg_sample)
from .gaussian import (FittedGBN, GaussianEvaluator, GaussianMomentsEvaluator, gaussian_cross_validate, gaussian_fit,  # noqa: F401
                       gaussian_joint, gaussian_log_likelihood, gaussian_predict, gaussian_sample)
from .gaussian_incomplete import (ExpectedMoments, GaussianConditioned, GaussianEMResult, expected_moments,  # noqa: F401
                                  gaussian_condition, gaussian_em_fit, gaussian_impute, gaussian_incomplete_log_likelihood,
                                  gaussian_posterior, incomplete_real_rows)
from .strength import (ArcStrength, AveragedNetwork, arc_strength, averaged_network, boot_strength, bootstrap_rows,  # noqa: F401
                       inclusion_threshold)

"""MI355X-native RBVAE hot path (gfx950): Python host side over librbvae_hip.so.

The directory name carries a hyphen (it mirrors the reference repository's name),
so import it with importlib -- `sfv_amd.py` at the repo root does that:

    import sfv_amd as sfv
    model = sfv.Seq2SeqBinaryVAE(in_channels=4, out_channels=4, latent_dim=32, variant="percep").cuda()
"""
from . import _lib  # noqa: F401
from .engine import VARIANTS, Engine, ParamLayout  # noqa: F401
from .losses import (contrast_loss, contrast_term, kl_binary_concrete, kl_binary_concrete_simple,  # noqa: F401
                     l1_loss, recon_loss, triplet_loss, triplet_term)
from .data import (DeviceStatePairDataset, assign_label, build_pairs, consistency_from_codes,  # noqa: F401
                   split_indices, state_consistency)
from .ldm import LDMDecoder, LDMEncoder, interpolate_embeddings  # noqa: F401
from .model import Seq2SeqBinaryVAE, binary_concrete_logits  # noqa: F401
from .trainer import FusedTrainer, noise_key  # noqa: F401
from .compose import OnTheFlyLatentTrainer  # noqa: F401
from .frames import (contrastive_input, extract_embeddings, load_frames, perturb_u8, resample_coeffs,  # noqa: F401
                     resize_u8, sd_input, to_reference_dict, u8_to_input)
from .robustness import (adjacent_hamming, most_common_codes, reference_draws, state_codes_under,  # noqa: F401
                         state_consistency_under)
from . import probe  # noqa: F401  (probe.split_indices is the probe's train/test split; data.split_indices the trainer's)
from .probe import ProbeResult, fit_factor, frame_embeddings, frame_probe, linear_probe  # noqa: F401
from . import projection  # noqa: F401
from .projection import (PCAResult, TSNEAffinities, TSNEResult, UMAPGraph, UMAPResult, fuzzy_csr,  # noqa: F401
                         fuzzy_graph, knn_graph, latent_projections, pca_project, tsne_affinities, tsne_project, umap_ab,
                         umap_optimise, umap_project)
from . import scores  # noqa: F401
from .scores import (continuity, knn_label_agreement, label_distance_sums, latent_scores, neighbour_ranks,  # noqa: F401
                     silhouette_samples, silhouette_score, trustworthiness)
from . import symbols  # noqa: F401
from .symbols import (KMeansResult, calinski_harabasz, cluster_sums, clustering_agreement, code_symbols,  # noqa: F401
                      contingency, davies_bouldin, kmeans, kmeans_plusplus, latent_symbols)
from . import mixture  # noqa: F401
from .mixture import (GMMResult, gmm, gmm_aic, gmm_bic, gmm_predict, gmm_predict_proba, gmm_score,  # noqa: F401
                      gmm_score_samples, gmm_select, latent_mixture)
from . import hmm as _hmm_module  # noqa: F401  (the module is sfv.hmm_model: the name hmm is the fit, as gmm is the mixture's)
from .hmm import (HMMResult, hmm, hmm_aic, hmm_bic, hmm_forward_backward, hmm_predict, hmm_predict_proba,  # noqa: F401
                  hmm_score, hmm_score_samples, hmm_select, hmm_sequence_scores, hmm_viterbi, latent_hmm, latent_hmm_videos)
hmm_model = _hmm_module
from . import bernoulli  # noqa: F401
from .bernoulli import (BHMMResult, BMMResult, bhmm, bhmm_aic, bhmm_bic, bhmm_predict, bhmm_predict_proba,  # noqa: F401
                        bhmm_score, bhmm_score_samples, bhmm_select, bmm, bmm_aic, bmm_bic, bmm_predict, bmm_predict_proba,
                        bmm_score, bmm_score_samples, bmm_select, latent_code_models, pack_codes)
from . import density  # noqa: F401
from .density import (DBSCANResult, dbscan, dbscan_sweep, k_distances, latent_density, noise_runs,  # noqa: F401
                      radius_graph, suggest_eps)
from .density import (HDBSCANResult, MSTResult, core_distances, hdbscan, hdbscan_cut, hdbscan_sweep,  # noqa: F401
                      latent_hdbscan, mutual_reachability_mst)
from . import segments  # noqa: F401
from .segments import (SegmentResult, SegmentTable, boundary_agreement, latent_segments, segment,  # noqa: F401
                       segment_layer, segment_prefix, segment_table)
from . import alignment  # noqa: F401
from .alignment import (DTWBarycenter, DTWResult, DTWTable, dtw, dtw_barycenter, dtw_distance_matrix,  # noqa: F401
                        dtw_fill, dtw_medoid, dtw_pairs, dtw_trace, latent_alignment, latent_alignment_videos,
                        transfer_labels, vote_labels, warp_map)
from . import spectral  # noqa: F401
from .spectral import (EigResult, NormalizedGraph, lanczos_eigsh, latent_spectral, normalized_graph,  # noqa: F401
                       spectral_clustering, spectral_embedding, spectral_layout)

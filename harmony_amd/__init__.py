"""harmony_amd -- MI355X-native implementation of Harmony's clustering + correction loop.

Host-side mirror of the reference's R API (RunHarmony / harmony_options / the `harmony` module
object) over the C ABI in include/harmony_mi355x.h.  All numerics run in hand-written HIP
(harmony_amd/csrc); there is no CPU fallback.
"""
from .doublets import doublet_neighbors, doublet_scores_from_counts, doublet_threshold, scrub_doublets, simulate_doublets
from .graph import connected_components, graph_connectivity, graph_from_knn, neighbors
from .group_stats import gene_stats_by_group, markers_from_sums, rank_genes_groups, variable_genes
from .harmony_obj import Harmony, HarmonyError
from .leiden import leiden
from .louvain import louvain
from .mapping import HarmonyReference, map_query, mapping_confidence
from .metrics import compute_lisi, knn, knn_predict, lisi_from_knn
from .options import harmony_options
from .pca import fit_loadings, gene_stats
from .project import HarmonyLoadings, map_query_counts, project_query
from .rank_sums import rank_sums_by_group, wilcoxon_from_rank_sums
from .silhouette import silhouette_batch, silhouette_label, silhouette_samples
from .snn import snn, snn_from_knn
from .ui import RunHarmony, prepare_setup_args
from .umap import find_ab_params, umap, umap_layout
from .umap_transform import umap_query_weights, umap_transform, umap_transform_from_knn
from .utils import harmonize

__all__ = ["RunHarmony", "harmony_options", "Harmony", "HarmonyError", "harmonize", "prepare_setup_args", "map_query",
           "HarmonyReference", "mapping_confidence", "knn", "compute_lisi", "lisi_from_knn", "knn_predict",
           "silhouette_samples", "silhouette_label", "silhouette_batch", "HarmonyLoadings", "project_query", "map_query_counts", "gene_stats", "fit_loadings",
           "gene_stats_by_group", "variable_genes", "rank_genes_groups", "markers_from_sums",
           "rank_sums_by_group", "wilcoxon_from_rank_sums", "neighbors", "graph_from_knn", "connected_components", "graph_connectivity",
           "snn", "snn_from_knn", "louvain", "leiden", "umap", "umap_layout", "find_ab_params",
           "umap_query_weights", "umap_transform_from_knn", "umap_transform",
           "simulate_doublets", "doublet_neighbors", "doublet_scores_from_counts", "doublet_threshold", "scrub_doublets"]

"""sharp_amd -- MI355X-native implementation of SHARP's ensemble random-projection +
meta-clustering hot path (reference: shibiaowan/SHARP, an R package).

Python mirror of the reference's exported R functions on that path; all compute runs
in libsharp_hip.so (hand-written HIP for gfx950) through its C ABI (include/sharp_hip.h)."""
from ._lib import SharpError, init, lib, reload_options, shutdown, so_path  # noqa: F401
from .api import *  # noqa: F401,F403
from .tsne import Rtsne, Rtsne_neighbors, knn, knn_descent  # noqa: F401
from .umap import UmapModel, knn_query, umap, umap_ab, umap_neighbors, umap_transform  # noqa: F401
from .tree import get_percluster_exp, hclust, plot_markers  # noqa: F401
from .validity import calinski_harabasz, cutree, silhouette  # noqa: F401
from .mapquality import continuity, knn_recall, neighbor_ranks, trustworthiness  # noqa: F401
from .community import louvain, louvain_graph, louvain_neighbors, louvain_snn, modularity  # noqa: F401
from .community import leiden, leiden_graph, leiden_neighbors, leiden_snn  # noqa: F401
from .diffmap import diffmap, diffmap_graph, diffmap_neighbors, dpt  # noqa: F401
from .snn import snn, snn_graph  # noqa: F401
from .expr_pca import expression_pca, expression_pca_transform, gene_stats  # noqa: F401
from .hvg import highly_variable_genes  # noqa: F401
from .harmony import batch_of_blocks, harmony_integrate  # noqa: F401
from .doublets import scrublet, simulate_doublets  # noqa: F401
from .rank_genes import rank_genes_groups  # noqa: F401
from . import dist  # noqa: F401,E402  (the multi-GPU module; calling it is R's dist() on the GPU, sharp_amd/tree.py)

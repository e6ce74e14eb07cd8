"""Single-device compute ops: HIP kernels (GPU) and native host kernels (CPU)."""
from .knn import (knn_cpu, finalize_cpu, merge_cpu, prepare_dataset, knn_gpu,  # noqa: F401
                  merge_gpu, finalize_gpu, format_report_gpu, DeviceDataset, DeviceResult,
                  vote_scores_cpu, vote_scores_gpu, class_proba, VOTE_SCORES_CMAX,
                  neighbor_means_cpu, neighbor_means_gpu, neighbor_means_curve_cpu,
                  neighbor_means_curve_gpu, curve_sse, NEIGHBOR_MEANS_TMAX, VOTE_WEIGHTS,
                  radius_count_cpu, radius_cpu, radius_count_gpu, radius_gpu,
                  radius_components_cpu, radius_components_gpu, exact_nearest_gpu)

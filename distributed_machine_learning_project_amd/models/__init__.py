"""Model front-ends (exact k-NN classifier and regressor, serial KD-tree, DBSCAN)."""
from .dbscan import DBSCAN  # noqa: F401
from .knn_classifier import KDTree, KNNClassifier  # noqa: F401
from .knn_regressor import KNNRegressor  # noqa: F401

# The drop-in provides data.graph_builder and data.negative_sampler; extend_path lets the reference's data.dataset and
# data.feature_extractor resolve from a later sys.path entry when this package comes first.
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)

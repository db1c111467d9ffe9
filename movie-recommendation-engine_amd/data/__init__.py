# The drop-in provides data.graph_builder only; extend_path lets the reference's data.dataset, data.feature_extractor and
# data.negative_sampler resolve from a later sys.path entry when this package comes first.
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)

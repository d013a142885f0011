from .field import WellField, ensemble_draw, forecast_sets, images  # noqa: F401
from .fit import likelihood_weights, quantise_weights  # noqa: F401

from .field import Allocation, SobolMaps, TimeToLimit, WellField, ensemble_draw, forecast_sets, images, sobol_design, worth_condition  # noqa: F401
from .fit import likelihood_weights, quantise_weights  # noqa: F401

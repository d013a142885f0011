from .field import TimeToLimit, WellField, ensemble_draw, forecast_sets, images, worth_condition  # noqa: F401
from .fit import likelihood_weights, quantise_weights  # noqa: F401

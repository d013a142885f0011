from .field import WellField, ensemble_draw, forecast_sets, images  # noqa: F401

from .field import WellField, forecast_sets, images  # noqa: F401

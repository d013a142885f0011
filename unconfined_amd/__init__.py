from .field import WellField, images  # noqa: F401

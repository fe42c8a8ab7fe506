from .metrics import Detection, MeanAveragePrecision, MAP  # noqa: F401
from .device import DeviceMeanAveragePrecision, GlobalResult  # noqa: F401
from .metrics import write_miss_rate_curves  # noqa: F401

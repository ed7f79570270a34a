from artiboost_amd.honet import HoNet  # noqa: F401  (anakin/models/honetMANO.py:20)

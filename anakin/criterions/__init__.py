from artiboost_amd.criterions import (AlignLoss, ChamferLoss, Criterion, HandOrdLoss, JointsLoss, ManoLoss, ObjLoss, SceneOrdLoss,  # noqa: F401
                                       SymCornerLoss)      # registers the eight LOSS types of anakin/criterions/__init__.py

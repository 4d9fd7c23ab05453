"""The dataset evaluator's second pixel measurement in numpy, the statement the full-size mode of csrc/af_quality.hip is checked
against: ``variance_of_laplacian(crop_rgb)`` of the crop as it is (altfreezing/TEST2.py:296-299, into ``_qstat``),

    lap = cv2.Laplacian(cv2.cvtColor(crop_rgb, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()

built on ``quality_ref``'s grey and Laplacian (the same restatement of OpenCV, without its INTER_AREA half-size stage) and pinned by
the two hand-worked crops of ``HAND_WORKED`` below (tests/test_runner_host.py checks them).
"""
import numpy as np

import quality_ref


def full_sums(crop: np.ndarray, channel_order: str = "rgb"):
    """``(n_px, S1, S2, grey image)`` of an HxWx3 uint8 crop at full size: Python integers and the (H, W) uint8 grey image"""
    g = quality_ref.grey(crop, channel_order)
    lap = quality_ref.laplacian(g)
    return int(g.size), int(lap.sum()), int((lap * lap).sum()), g


def full_variance(crop: np.ndarray, channel_order: str = "rgb") -> float:
    n, s1, s2, _ = full_sums(crop, channel_order)
    return quality_ref.variance(n, s1, s2)


def min_side_and_full_lap(crop: np.ndarray, channel_order: str = "rgb"):
    """what ``_qstat`` records of a crop"""
    return float(min(crop.shape[:2])), full_variance(crop, channel_order)


def _grey_crop(values) -> np.ndarray:
    """a crop with R = G = B = v: its grey byte is (v * 32768 + 16384) >> 15 = v"""
    v = np.asarray(values, dtype=np.uint8)
    return np.repeat(v[..., None], 3, axis=2)


# (crop, n_px, S1, S2) worked by hand:
#   1 x 5, grey 10 20 40 80 160: the one row is its own upper and lower neighbour, so L = left + right - 2 * centre with the columns
#     reflected (-1 -> 1, 5 -> 3): 20 + 20 - 20 = 20, 10 + 40 - 40 = 10, 20 + 80 - 80 = 20, 40 + 160 - 160 = 40, 80 + 80 - 320 = -160;
#     S1 = -70, S2 = 400 + 100 + 400 + 1600 + 25600 = 28100, variance (5 * 28100 - 4900) / 25 = 5424
#   3 x 3, grey 1 2 3 / 4 5 6 / 7 8 10: L = 8 6 4 / 2 0 -1 / -4 -5 -12 (corner (0, 0): 4 + 4 + 2 + 2 - 4; centre: 2 + 8 + 4 + 6 - 20;
#     corner (2, 2): 6 + 6 + 8 + 8 - 40); S1 = -2, S2 = 64 + 36 + 16 + 4 + 0 + 1 + 16 + 25 + 144 = 306, variance (9 * 306 - 4) / 81
HAND_WORKED = [
    (_grey_crop([[10, 20, 40, 80, 160]]), 5, -70, 28100),
    (_grey_crop([[1, 2, 3], [4, 5, 6], [7, 8, 10]]), 9, -2, 306),
]

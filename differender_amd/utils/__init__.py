from .utils import get_tf, in_circles, get_rand_pos, tex_from_pts
from .losses import (ssim2d, dssim_mse_loss, fused_dssim_mse_loss, MS_SSIM_WEIGHTS, ms_ssim2d, ms_dssim_mse_loss,
                     fused_ms_dssim_mse_loss, tv3d, fused_tv3d_loss)

"""Calibrations the undistortion tests share: the three shipped ones (Extras/Calib/EuRoC.yaml,
TumMono_20-27-33-34.yaml, Kitti00to02.yaml) restated as settings, and small ones of the same models."""
import numpy as np

EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
# a public 512 x 512 fisheye calibration of the equidistant family (its four coefficients serve both fisheye models)
FISHEYE_K = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504)
FISHEYE_DIST = (0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)

CASES = {
    "kitti": dict(model="Pinhole", w_in=1241, h_in=376, w_out=1232, h_out=368,
                  K_in=(7.18856e+02, 7.18856e+02, 6.071928e+02, 1.852157e+02), dist=(0.0,), process="crop"),
    "euroc": dict(model="RadTan", w_in=752, h_in=480, w_out=640, h_out=480,
                  K_in=(458.654, 457.296, 367.215, 248.375), dist=EUROC_DIST, process="useK",
                  desired_K=(0.6, 0.9, 0.5, 0.5)),
    "small_crop": dict(model="RadTan", w_in=96, h_in=64, w_out=64, h_out=48, K_in=(60.0, 60.0, 47.5, 31.5),
                       dist=EUROC_DIST, process="crop"),
    "small_usek": dict(model="RadTan", w_in=96, h_in=64, w_out=64, h_out=48, K_in=(60.0, 60.0, 47.5, 31.5),
                       dist=EUROC_DIST, process="useK", desired_K=(0.45, 0.6, 0.5, 0.5)),
    "odd_crop": dict(model="RadTan", w_in=101, h_in=67, w_out=61, h_out=45, K_in=(63.0, 62.0, 50.0, 33.0),
                     dist=EUROC_DIST, process="crop"),
    "none": dict(model="Pinhole", w_in=64, h_in=48, w_out=64, h_out=48, K_in=(40.0, 40.0, 31.5, 23.5), dist=(0.0,),
                 process="none"),
    "chain": dict(model="RadTan", w_in=352, h_in=264, w_out=320, h_out=240, K_in=(215.0, 214.0, 175.5, 131.5),
                  dist=EUROC_DIST, process="useK", desired_K=(0.55, 0.73, 0.5, 0.5)),
    # tolerance cases (libm against numpy in atan / tan): useK only
    "tum": dict(model="Atan", w_in=1280, h_in=1024, w_out=640, h_out=480,
                K_in=(0.349153, 0.436593, 0.49314, 0.499021), dist=(0.933271,), process="useK",
                desired_K=(0.4, 0.53, 0.5, 0.5)),
    "equi": dict(model="EquiDistant", w_in=512, h_in=512, w_out=256, h_out=256, K_in=FISHEYE_K, dist=FISHEYE_DIST,
                 process="useK", desired_K=(0.4, 0.4, 0.5, 0.5)),
    "kb": dict(model="KannalaBrandt", w_in=512, h_in=512, w_out=256, h_out=256, K_in=FISHEYE_K, dist=FISHEYE_DIST,
               process="useK", desired_K=(0.4, 0.4, 0.5, 0.5)),
}


def lib_calib(name):
    from hslam_amd.undistort import make_calib
    c = CASES[name]
    return make_calib(c["model"], c["w_in"], c["h_in"], c["w_out"], c["h_out"], c["K_in"], c["dist"], c["process"],
                      c.get("desired_K", (0.0, 0.0, 0.0, 0.0)))


def ref_remap(name, **kw):
    import undist_ref
    c = CASES[name]
    return undist_ref.make_remap(c["model"], c["w_in"], c["h_in"], c["w_out"], c["h_out"], c["K_in"], c["dist"],
                                 c["process"], c.get("desired_K"), **kw)


def gamma_G():
    return (((np.arange(256) / 255.0) ** 0.8) * 200 + 3).astype(np.float32)


def random_vignette(shape, seed=3):
    return np.random.default_rng(seed).integers(20000, 65536, size=shape, dtype=np.uint16)

"""The parity cases of d2d_nlp_guess_dubins (tests/test_nlp_guess_cpu.py asserts what this table claims and that every case is
DETERMINED; tests/test_gpu_nlp_guess.py compares the kernel with the statement on them).  Built on the CPU by a random search over
five families -- perturbed exp_14, far and near end poses with random headings, a goal dead ahead 4 .. 5 mm beside the axis, more than
a full turn between the end headings -- kept where the determinacy rule holds at every node count with a factor 10 to spare.

A case: (p0, p1, drift (D2D_SC_WX, D2D_SC_WY), KV, VREF, its row of opts.bounds, its v_pref, then (status, word) of the 'plain' launch
-- no bounds, v_pref NULL -- and of the 'opts' launch -- both arrays).  VSP = 12, v in [9, 15], PHIMAX = 0.6981 in every row.  Every
launch has the duration T0 = 12 s: h = T0 / (N - 1), so a case keeps its status and word at every node count."""
import numpy as np

import nlp_guess_ref as GR

T0 = 12.0
NS = (2, 3, 5, 64, 65, 121, 129)
BS = (1, 63, 65)
VARIANTS = ('plain', 'opts')
V_BOX, PHIMAX, VSP = (9.0, 15.0), 0.6981, 12.0
STRIDE = 80                         # d2dhip.SCEN_STRIDE (tests/test_nlp_guess_cpu.py compares)
F_MIN, MARGIN_MIN = 1e-9, 1e-6      # determinacy: no search evaluation with |F| < F_MIN v T; the second-best word MARGIN_MIN longer, relative

CASES = (
    ((-15.761, -8.812, 1.368), (-161.673, 26.193, 3.606), (0.0, 0.0), 0.0, 0.0, (-0.7, 0.55, -9.0, 9.0), 15.06, (0, 0), (1, 0)),
    ((-16.756, 54.247, -2.275), (-128.721, -38.855, -2.583), (0.0, 0.0), 1.0, 13.0, (-0.6, 0.75, 0.0, 0.0), 13.98, (0, 1), (2, 3)),
    ((-50.741, -58.97, 2.182), (72.258, 40.657, 0.108), (-0.06, 0.59), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 12.17, (0, 1), (1, 1)),
    ((31.852, -24.698, -1.918), (46.419, -165.343, -2.524), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 14.85, (0, 2), (2, 2)),
    ((-41.651, -23.761, -0.565), (60.186, -103.716, 1.184), (0.0, 0.0), 1.0, 13.0, (-0.6, 0.75, 0.0, 0.0), 10.1, (0, 3), (0, 3)),
    ((-47.525, -59.682, 2.299), (72.605, 41.071, 0.171), (-0.8, 2.87), 0.0, 0.0, (-0.7, 0.55, -9.0, 9.0), 14.85, (0, 3), (1, 3)),
    ((35.752, -14.343, 1.28), (-71.381, 27.296, 5.213), (0.0, 0.0), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 14.16, (1, 0), (1, 0)),
    ((53.973, -56.516, 1.02), (141.027, -181.33, -1.516), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 10.99, (1, 1), (1, 1)),
    ((-50.974, -60.661, 2.365), (76.705, 47.295, 0.064), (1.11, -0.22), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 12.99, (1, 1), (1, 1)),
    ((-47.149, 23.067, 0.812), (-70.671, 97.812, -1.635), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 11.23, (1, 2), (1, 5)),
    ((-5.535, 31.005, 0.833), (-1.889, 34.779, 0.165), (2.56, 1.4), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 13.76, (1, 2), (1, 2)),
    ((56.902, 47.721, 2.065), (137.647, 44.179, 3.479), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 8.93, (1, 3), (1, 3)),
    ((-49.498, -58.992, 2.348), (74.753, 44.183, 0.15), (-2.13, 2.67), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 13.39, (1, 3), (1, 3)),
    ((6.672, -27.426, 2.278), (19.564, -0.389, 5.239), (0.0, 0.0), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 14.77, (1, 4), (1, 4)),
    ((-58.707, -33.633, -0.253), (-57.215, -41.261, 0.46), (-0.74, -0.95), 1.0, 13.0, (-0.6, 0.75, 0.0, 0.0), 10.14, (1, 4), (1, 4)),
    ((58.844, 29.575, 2.732), (120.317, 6.784, 0.823), (0.0, 0.0), 0.0, 0.0, (-0.7, 0.55, -9.0, 9.0), 8.62, (1, 5), (1, 5)),
    ((44.663, -57.778, 1.245), (46.709, -57.735, 1.055), (-1.78, -1.05), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 14.14, (1, 5), (1, 5)),
    ((51.374, 46.767, -0.117), (96.457, 125.225, 2.753), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 10.86, (2, 0), (2, 0)),
    ((-52.534, -54.463, -2.381), (-150.859, 23.882, -5.131), (0.0, 0.0), 1.0, 11.0, (-0.6, 0.75, 0.0, 0.0), 14.41, (2, 1), (2, 1)),
    ((-48.667, -54.45, 2.082), (72.22, 36.852, 0.017), (1.76, -0.72), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 11.62, (2, 1), (0, 1)),
    ((-22.026, -42.115, 1.191), (11.8476, 42.774, 1.1911), (0.0, 0.0), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 10.15, (2, 2), (2, 2)),
    ((-41.656, 25.547, 2.086), (-25.366, 31.21, 2.024), (2.75, -1.1), 1.0, 13.0, (-0.6, 0.75, 0.0, 0.0), 11.31, (2, 2), (2, 2)),
    ((-59.89, -9.578, 0.789), (28.5319, 79.409, 0.7886), (0.0, 0.0), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 10.79, (2, 3), (2, 3)),
    ((-48.719, -54.732, 2.231), (73.342, 37.646, 0.075), (3.0, 0.91), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 11.54, (2, 3), (2, 1)),
    ((7.565, -0.986, 0.691), (62.859, 17.99, 2.07), (0.0, 0.0), 1.0, 13.0, (-0.6, 0.75, 0.0, 0.0), 9.84, (2, 4), (2, 4)),
    ((19.413, 26.826, -2.497), (-7.079, 10.141, -1.072), (2.32, -0.1), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 12.69, (2, 4), (1, 4)),
    ((-43.839, 52.166, 2.567), (-61.325, 88.611, -0.771), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 11.23, (2, 5), (2, 5)),
    ((-3.86, 16.122, 0.466), (20.507, 9.167, -1.031), (-0.25, 2.24), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 12.89, (2, 5), (1, 5)),
    ((55.491, 23.794, -1.992), (25.5851, -42.9644, -1.9919), (0.0, 0.0), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 15.08, (3, 0), (2, 3)),
    ((-29.412, -5.359, 1.346), (-8.8894, 84.3537, 1.3458), (0.0, 0.0), 0.0, 11.0, (-0.7, 0.55, -9.0, 9.0), 13.8, (3, 1), (2, 2)),
    ((-16.031, -9.991, 1.082), (37.9443, 91.5202, 1.0821), (0.0, 0.0), 0.0, 13.0, (-0.7, 0.55, -9.0, 9.0), 11.13, (3, 2), (3, 2)),
    ((-31.136, -9.712, 1.09), (15.3233, 79.3247, 1.0898), (0.0, 0.0), 0.0, 0.0, (-0.7, 0.55, -9.0, 9.0), 13.48, (3, 3), (2, 3)),
    ((-21.626, 35.986, 0.042), (-29.895, -59.103, 7.462), (0.0, 0.0), 1.0, 0.0, (-0.6, 0.75, 0.0, 0.0), 9.1, (4, -1), (4, -1)),
)


def step(N):
    return T0 / (N - 1)


def row(case):
    p0, p1, w, kv, vref = case[:5]
    r = np.zeros(STRIDE)
    r[GR.SC_X0:GR.SC_X0 + 3], r[GR.SC_X1:GR.SC_X1 + 3] = p0, p1
    r[GR.SC_WX], r[GR.SC_WY] = w
    r[GR.SC_VMIN], r[GR.SC_VMAX] = V_BOX
    r[GR.SC_PHIMAX], r[GR.SC_VSP], r[GR.SC_KV], r[GR.SC_VREF] = PHIMAX, VSP, kv, vref
    return r


def batch(B, variant):
    """The first B cases, cycled: rows [B][STRIDE], bounds [B][4] and v_pref [B] (None, None for 'plain'), expected (status, word) [B]."""
    cs = [CASES[b % len(CASES)] for b in range(B)]
    rows = np.stack([row(c) for c in cs])
    want = np.array([c[7 if variant == 'plain' else 8] for c in cs], np.int32)
    if variant == 'plain':
        return rows, None, None, want
    return rows, np.array([c[5] for c in cs], float), np.array([c[6] for c in cs], float), want


def one(case, variant, N, trace=None):
    opts = variant == 'opts'
    return GR.guess_one(row(case), N, step(N), case[5] if opts else None, case[6] if opts else None, trace=trace)


def determined(case, variant, N):
    """The determinacy rule for one parity case: (smallest |F| / (v T) over the search evaluations, smallest relative margin of the
    second-best admissible word at the bracket ends and at the result); inf where there is none."""
    tr = []
    one(case, variant, N, tr)
    return (min([x for k, x in tr if k == 'F'], default=np.inf), min([x for k, x in tr if k == 'margin'], default=np.inf))


# rows that are refused (D2D_GUESS_INVALID): (column or name, value) put into case 0's row
REFUSALS = ((GR.SC_X0, np.nan), (GR.SC_X1 + 2, np.inf), (GR.SC_WX, np.nan), (GR.SC_VMIN, 0.0), (GR.SC_VMIN, 16.0), (GR.SC_VMAX, np.inf),
            (GR.SC_PHIMAX, 0.0), (GR.SC_PHIMAX, 1.6), (GR.SC_PHIMAX, np.nan), (GR.SC_KV, np.nan), (GR.SC_VSP, np.inf))


def refused_rows():
    out = []
    for col, val in REFUSALS:
        r = row(CASES[0])
        r[col] = val
        out.append(r)
    return np.stack(out)

"""Rosenbrock-Wanner coefficient tables.

The numbers are the literals of the reference (``triflow/core/schemes.py``:
ROS2 ``:250-256``, ROS3PRw ``:278-300``, ROS3PRL ``:322-353``, RODASPR
``:375-427``) -- including RODASPR's gamma entries, which are written there
with 7-9 significant digits and must be reproduced as such to match its
trajectories.  ``gamma[i, i]`` is the same for every stage of a scheme (one
factorisation of ``I - gamma_ii dt J`` per step).
"""

from collections import namedtuple

import numpy as np

Tableau = namedtuple("Tableau", "alpha gamma b b_pred")


def _lower(s, entries):
    a = np.zeros((s, s))
    for (i, j), v in entries.items():
        a[i, j] = v
    return a


def _make():
    tabs = {}

    tabs["ROS2"] = Tableau(
        alpha=np.array([[0., 0.], [1., 0.]]),
        gamma=np.array([[2.928932188134E-1, 0.],
                        [-5.857864376269E-1, 2.928932188134E-1]]),
        b=np.array([1 / 2, 1 / 2]),
        b_pred=None)

    g = 7.8867513459481287e-01
    tabs["ROS3PRw"] = Tableau(
        alpha=_lower(3, {(1, 0): 2.3660254037844388e+00,
                         (2, 0): 5.0000000000000000e-01,
                         (2, 1): 7.6794919243112270e-01}),
        gamma=_lower(3, {(0, 0): g, (1, 1): g, (2, 2): g,
                         (1, 0): -2.3660254037844388e+00,
                         (2, 0): -8.6791218280355165e-01,
                         (2, 1): -8.7306695894642317e-01}),
        b=[5.0544867840851759e-01, -1.1571687603637559e-01,
           6.1026819762785800e-01],
        b_pred=[2.8973180237214197e-01, 1.0000000000000001e-01,
                6.1026819762785800e-01])

    g = 4.3586652150845900e-01
    tabs["ROS3PRL"] = Tableau(
        alpha=_lower(4, {(1, 0): .5, (2, 0): .5, (2, 1): .5,
                         (3, 0): .5, (3, 1): .5, (3, 2): 0}),
        gamma=_lower(4, {(0, 0): g, (1, 1): g, (2, 2): g, (3, 3): g,
                         (1, 0): -5.0000000000000000e-01,
                         (2, 0): -7.9156480420464204e-01,
                         (2, 1): 3.5244216792751432e-01,
                         (3, 0): -4.9788969914518677e-01,
                         (3, 1): 3.8607515441580453e-01,
                         (3, 2): -3.2405197677907682e-01}),
        b=[2.1103008548132443e-03, 8.8607515441580453e-01,
           -3.2405197677907682e-01, 4.3586652150845900e-01],
        b_pred=[5.0000000000000000e-01, 3.8752422953298199e-01,
                -2.0949226315045236e-01, 3.2196803361747034e-01])

    g = .25
    tabs["RODASPR"] = Tableau(
        alpha=_lower(6, {(1, 0): 7.5E-1,
                         (2, 0): 7.5162877593868457E-2,
                         (2, 1): 2.4837122406131545E-2,
                         (3, 0): 1.6532708886396510e0,
                         (3, 1): 2.1545706385445562e-1,
                         (3, 2): -1.3157488872766792e0,
                         (4, 0): 1.9385003738039885e1,
                         (4, 1): 1.2007117225835324e0,
                         (4, 2): -1.9337924059522791e1,
                         (4, 3): -2.4779140110062559e-1,
                         (5, 0): -7.3844531665375115e0,
                         (5, 1): -3.0593419030174646e-1,
                         (5, 2): 7.8622074209377981e0,
                         (5, 3): 5.7817993590145966e-1,
                         (5, 4): 2.5e-1}),
        gamma=_lower(6, {(0, 0): g, (1, 1): g, (2, 2): g,
                         (3, 3): g, (4, 4): g, (5, 5): g,
                         (1, 0): -7.5e-1,
                         (2, 0): -8.8644e-2, (2, 1): -2.868897e-2,
                         (3, 0): -4.84700e0, (3, 1): -3.1583e-1,
                         (3, 2): 4.9536568e0,
                         (4, 0): -2.67694569e1, (4, 1): -1.5066459e0,
                         (4, 2): 2.720013e1, (4, 3): 8.25971337e-1,
                         (5, 0): 6.58762e0, (5, 1): 3.6807059e-1,
                         (5, 2): -6.74235e0, (5, 3): -1.061963e-1,
                         (5, 4): -3.57142857e-1}),
        b=[-7.9683251690137014E-1, 6.2136401428192344E-2,
           1.1198553514719862E00, 4.7198362114404874e-1,
           -1.0714285714285714E-1, 2.5e-1],
        b_pred=[-7.3844531665375115e0, -3.0593419030174646e-1,
                7.8622074209377981e0, 5.7817993590145966e-1, 2.5e-1, 0])
    return tabs


TABLEAUX = _make()


#: Explicit Runge-Kutta tableaux (``schemes.ERK_general``): ``a`` strictly lower triangular, ``b`` the
#: weights of the solution that is propagated, ``b_err`` those of the embedded lower-order solution (None:
#: fixed step only), ``order`` that of the propagated solution.  The literals are exact fractions evaluated
#: in double.
ERKTableau = namedtuple("ERKTableau", "a b b_err order")


def _make_erk():
    tabs = {}

    # Shu & Osher (1988): the optimal strong-stability-preserving scheme of three stages
    tabs["SSPRK3"] = ERKTableau(
        a=_lower(3, {(1, 0): 1., (2, 0): 1 / 4, (2, 1): 1 / 4}),
        b=np.array([1 / 6, 1 / 6, 2 / 3]), b_err=None, order=3)

    tabs["RK4"] = ERKTableau(
        a=_lower(4, {(1, 0): 1 / 2, (2, 1): 1 / 2, (3, 2): 1.}),
        b=np.array([1 / 6, 1 / 3, 1 / 3, 1 / 6]), b_err=None, order=4)

    # Bogacki & Shampine (1989), 3(2); the fourth stage is F at the new state
    tabs["BS23"] = ERKTableau(
        a=_lower(4, {(1, 0): 1 / 2, (2, 1): 3 / 4, (3, 0): 2 / 9, (3, 1): 1 / 3, (3, 2): 4 / 9}),
        b=np.array([2 / 9, 1 / 3, 4 / 9, 0.]),
        b_err=np.array([7 / 24, 1 / 4, 1 / 3, 1 / 8]), order=3)

    # Dormand & Prince (1980), 5(4); the seventh stage is F at the new state
    tabs["DOPRI5"] = ERKTableau(
        a=_lower(7, {(1, 0): 1 / 5,
                     (2, 0): 3 / 40, (2, 1): 9 / 40,
                     (3, 0): 44 / 45, (3, 1): -56 / 15, (3, 2): 32 / 9,
                     (4, 0): 19372 / 6561, (4, 1): -25360 / 2187, (4, 2): 64448 / 6561,
                     (4, 3): -212 / 729,
                     (5, 0): 9017 / 3168, (5, 1): -355 / 33, (5, 2): 46732 / 5247,
                     (5, 3): 49 / 176, (5, 4): -5103 / 18656,
                     (6, 0): 35 / 384, (6, 2): 500 / 1113, (6, 3): 125 / 192,
                     (6, 4): -2187 / 6784, (6, 5): 11 / 84}),
        b=np.array([35 / 384, 0., 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.]),
        b_err=np.array([5179 / 57600, 0., 7571 / 16695, 393 / 640, -92097 / 339200,
                        187 / 2100, 1 / 40]), order=5)
    return tabs


ERK_TABLEAUX = _make_erk()

"""Colour tables of the rendered one-channel outputs: the 256 x 3 float32 tables of matplotlib's listed colormaps that nerfstudio's
``apply_float_colormap`` indexes (``matplotlib.colormaps[name].colors``), plus ``gray`` (i / 255) and ``default`` (= ``turbo``,
nerfstudio's choice for one-channel floats).

The tables are DATA: the float32 values of matplotlib 3.10.8, little-endian, base64.  They are stored here so that rendering needs no
matplotlib; tests/test_render_cpu.py compares them with the installed matplotlib when there is one."""
from __future__ import annotations

import base64
from typing import Dict

import numpy as np
import torch

NAMES = ("default", "turbo", "viridis", "magma", "inferno", "plasma", "cividis", "gray")

_B64 = {
    "turbo": (
        "QYJCPuj2kj35vW0+hIFHPmDIqj0E4oU+dVlMPuCEwj1WmpQ+swxRPign2j2RCqM+PZtVPni08T0WMLE+FAVaPsmTBD41DL8+OEpePjpAED6dncw+qWpiPi7i"
        "Gz6f5dk+ZmZmPgh3Jz475OY+cT1qPmUBMz5wmfM+yO9tPqZ+Pj6fAgA/zHpxPszuST4rEwY/veN0PnZUVT4E/ws/+id4PgStYD6CxRE/hEd7Pnf4az5NZxc/"
        "W0J+Pm05dz5l5Bw/P4yAPqQ2gT7JPCI/qOOBPlPLhj56cCc/BiqDPnVZjD7Qfiw/C16EPgnhkT5zaDE/t3+FPl5jlz66LDY/uY2GPibfnD5PzDo/sYqHPrBV"
        "oj4wRz8/T3WIPqzFpz5enUM/REyJPhsvrT7Zzkc/MBKKPkuTsj752ks/csSKPu3wtz5lwk8/qmWLPlJJvT53hFM/OPOLPtmZwj59Ilc/vW+MPnHmxz4om1o/"
        "mdiMPiwrzT547l0/ajCNPqlq0j69HWE/knSNPuik1z6mJ2Q/saeNPpnY3D7dDGc/JseNPrwF4j64zGk/QdSNPqEt5z6IaGw/U9CNPqlN7D783m4/u7iNPsJp"
        "8T4WMHE/yY6NPk5/9j4lXXM/zlONPkyO+z7YZHU/KQWNPl5LAD/YR3c/K6SMPvfMAj8lBnk/0zCMPvFLBT8Xn3o/RKOLPkvIBz9nD3w/YMiKPkVHCj/EQn0/"
        "iJ2JPobJDD83N34/qyaIPmZODz+37n4/BWmGPuXVET88a38/12mEPltfFD+8rn8/Di2CPnnpFj/Yu38/cXJ/Pj90GT/ek38/6iF6Pqz/Gz9tOX8/Qnh0PhqL"
        "Hj99rn4/GHhuPjgVIT8G9X0/xjNoPgaeIz/+Dn0/661hPoUlJj8E/3s/ofNaPg2rKD9pxno/yAxUPk0tKz8jZ3k/2gNNPu+sLT965Hc/8+VFPqIoMD8UP3Y/"
        "Urg+Pr6fMj+SeXQ/Eog3PuwSNT+SlnI/EF0wPjSANz9jl3A/yEEpPj7oOT/+fW4/GD4iPmJKPD8BTWw/HF8bPvilPj9kBmo/sKwUPrH5QD91q2c/UTEOPjVG"
        "Qz99P2U/e/cHPtuKRT/Kw2I/DAcCPlTGRz/7OmA/PNr4PUj5ST+5pV0/4V3uPWgiTD/yB1s/PrPkPbNBTj9OYlg/DOrbPdpVUD8TuFU/ghzUPYVfUj/qCVM/"
        "HVXNPWRdVD8YW1A/FK7HPc9OVj/vrE0/IjfDPW40WD9lAUs/fArAPUoMWj8YW0g/oDK+PQrXWz8CvEU/xcm9PQiUXT8YJkM/pN++PZpCXz9Sm0A/dY7BPXLh"
        "YD9PHj4/teDFPTdxYj9gsDs/mfDLPUHxYz96Uzk/3c3TPUJgZT89Cjc/v33dPXbDZj/DuzQ/hPDoPXUfaD97TjI/9gv2PT90aT8FxS8/zGICPivBaj8IIC0/"
        "mYEKPjoGbD8kYio/JV0TPsRCbT8AjCc/U+gcPnB3bj/koCQ/SBsnPpijbz93oSE/w/AxPpPGcD+wjx4/DFk9PgnhcT/fbBs/5E5JPlLycj+jOxg/zsdVPm76"
        "cz9M/RQ/7btiPrb4dD8psxE/Jh5wPintdT8xXw4/2et9PsfXdj8EBAs/pgqGPum3dz+hoQc/8UuNPjeOeD9POwQ/7rGUPghaeT9f0gA/ADqcPrUaej8+0Po+"
        "6N6jPj7Qej8N/fM+Z5urPqJ6ez8bL+0+kGuzPuMZfD8FaeY+c0u7PlitfD+8rt8+0jXDPgE1fT8uBNk+wCbLPt6wfT/4a9I+rRfTPkcgfj+86Ms++wXbPjyD"
        "fj8GgcU+bOziPr7Zfj/XNL8+wcXqPiUjfz9sCbk+XI/yPnBffz+0ArM+r0L6PkePfz9PI60+Pu0AP7Swfz/bbac+EaoEPwXFfz+W56E+MlUIP+rKfz8hk5w+"
        "q+wLPw3Dfz9pdJc+M20PP8Wsfz+9jJI+fNUSPxKIfz+s4o0+PiIWP/NUfz+Fd4k+KlIZP8ISfz+HUIU+omIcP3/Bfj8Ab4E+BVEfP4Bgfj9gsHs+XBsiP2/w"
        "fT9pHXU+SMQkP/xvfT9aKm8+nWgnPy/dfD+V1Gk+QQ4qP7A4fD+dEWU+5bMsP4CCez/T3mA+OlgvP526ej9ZNF0+5/sxP7HheT/yDFo+nZ00Pwn5eD8gXlc+"
        "tDw3PwAAeD9GJVU+hNg5P5T2dj+GWlM+DXE8P77edT8B9lE+/wQ/P9S3dD8b9VA+W5RBP4CCcz/0T1A+0h1EP8A+cj8R/E8+CqJGP+XtcD9y+U8+DB9JP++P"
        "bz+bPVA+2ZRLP90kbj+twFA+yQJOP1itbD8KgFE+3GhQPwYqaz/Wc1I+wcVSP5GbaT/RllM+0hhVP1ABaD9/3lQ+Z2FXPzpdZj9BSFY+J6BZPwCuZD86zFc+"
        "dNJbP/H0Yj8sZVk+nPldP7UyYT85C1s+qRNgP01nXz8kuVw+myBiP2CTXT8OZ14+cSBkP+22Wz8bDWA+NBFmP57SWT9Lq2E+5fJnPxnnVz+DNGM+gsVpP170"
        "VT+Do2Q+vodrP737Uz8O82U+lzltP+f7UT/nHWc+vtluP9P2Tz8uHGg+NGhwP4HsTT8I5mg+UORxP/DcSz/VeGk+wkxzP3HJST8Zymk+NKJ0P1uxRz8012k+"
        "rOJ1P1eVRT+rlWk+1A53Pwx2Qz8/AGk+syR4PyJUQT+yEWg+miV5P5gvPz/GxGY+6Q56PxgJPT/+DmU+SOF6P0jhOj+77WI+rp57P6ytOD+5cGA+E0l8P2Zm"
        "Nj8tsl0+HuF8P3gLND+3tFo+d2d9PzCeMT/2elc+d9t9P94fLz+JB1Q+bD5+P4KQLD8QXVA+sI9+P7vyKT/HgEw+Qs9+P+FFJz/ud0g+cv5+P5OMJD/mP0Q+"
        "Px1/PyrGIT+L4D8+Ait/P0X1Hj99XDs+Cyl/P+MZHD+8szY+sRZ/P600GT8k7jE+RfV+P5lHFj+3Cy0+dsN+P1BTEz8TDyg+PIN+PyFZED8VACM+SDN+PwxZ"
        "DT++3h0+6dR9PwhVCj+srRg+H2h9P2ZOBz9+bxM+6ux8P3xEBD90KQ4+8WN8P+s5AT/K4Ag+Ns17P7Ne/D7ikgM+Dyh7P+BK9j4yj/w9dXZ6P/s68D4dA/I9"
        "F7d5P1Uw6j7Chuc9Rut4Pz0s5D5gH909ARN4P/Az3j410tI9SS53PyBG2D69qcg9HT12P2tl0j42q749JUB1P8CVzD7g27Q9CTh0Px/Xxj72QKs9ICRzPygs"
        "wT735KE9bARyPymWuz4hzZg95NpwPxEZtj6w/o89j6VvP+G0sD7lfoc9ZmZuP4dtqz51sH49aR1tPwNDpj5iFW8978lrP0M5oT6JQWA9oGxqP0hQnD7kSVI9"
        "fQVpPwCMlz5zLkU91ZVnP2zskj6x+Tg9AB1mP3l1jj4Uyy09VppkP4kkij6kjSM9iQxjP/PlhT4PuRk973JhP8i1gT5cOBA94sxfP3Alez6NCwc9CRteP8X+"
        "cj46evw8vFxcP/H0aj4fhes8o5JaP1MFYz7CTNs8F7xYPys1Wz4svMs8vtlWPzl/Uz5b07w8mutUPx3mSz5Pkq48AvFSP3ZsRD4CDqE8nupQPwYNPT57MZQ8"
        "b9hOP23KNT65/Ic8y7lMP6mkLj5sCXk8XI9KP7ubJz7/PmM8eVhIP0KyID4BGE88yhVGPwDjGT6cFjw8UMdDP5QwEz60jio8YWxBP/6aDD5YVho8/wQ/P58f"
        "Bj6HbQs8eZI8P2qH/z1l/Ps7fxM6P0IJ8z3TvOM7Eog3P8bE5j1YHM472PA0P/W52j30Grs7000yP5Pjzj2JDKs7Ap8vPxtMwz00nZ07veMsPxDptz3aIJM7"
        "BBwqP/DErD2z74o7gEgnPz3VoT2FsYU7L2kkP3Qklz1RZoM7a30hPxqojD1RZoM724UeP2tlgj1LWYY7gIIbP0zDcD1b64s7sHIYP54kXT1lcJQ7FVcVP0j5"
        "ST2jQJ87Bi8SP0pBNz28V607K/sOP6T8JD0Kur07hLsLP1YrEz1SD9E7aW8IP2DNAT2wA+c7gxcFP4LF4Twkl/87KbMBP/XWwDzYZA08BYb8PhjPoDyadxw8"
        "Io71PuutgTzo2Sw8"
    ),
    "viridis": (
        "wLSIPhO2nzsVqag+JXqJPkpeHTwWvas+GjaKPrKdbzw6ya4+feiKPmhdozw+zbE+cZGLPn9p0TybyLQ+sTCMPgADAT2Vu7c+gsaMPtehGj1hpbo+wVKNPnXo"
        "ND0jhr0+TtWNPoM1Tj23XcA+SE6OPv+zZj13K8M+sr2OPsGLfj1j78U+RiOPPprtij1Yqcg+KH+PPqdblj3zWMs+V9GPPv6ZoT0R/s0+sRmQPvevrD2RmNA+"
        "WFiQPs+itz0PKNM+Ko2QPsR3wj1prNU+SriQPo8zzT1bJdg+lNmQPknY1z3mkto+TvGQPpxp4j2l9Nw+Mv+QPqPp7D13St8+ZAORPu9Z9z06lOE+4/2QPkze"
        "AD7M0eM+0O6QPlcJBj7rAuY+LNaQPp0uCz6VJ+g+9rOQPuhOED6rP+o+UYiQPvVpFT4KS+w+flOQPo2AGj6QSe4+PBWQPvOSHz4dO/A+7s2PPiehJD7RH/I+"
        "lX2PPm2rKT6M9/M+UySPPoGxLj4rwvU+SMKOPqezMz7Qf/c+l1eOPiCyOD5ZMPk+guSNPmmsPT7p0/o+TWmNPsKiQj6havw+1uWMPi2VRz5e9P0+gVqMPqmD"
        "TD5Dcf8+cceLPrFtUT7KcAA/Ci2LPodTVj6WIgE/bouKPuc0Wz4pzgE/veKJPtMRYD6jcwI/GjOJPgfqZD71EgM/LH2IPoS9aT5grAM/FsGHPgWMbj7VPwQ/"
        "1v6GPopVcz6WzQQ/9DaGPtIZeD6TVQU/kGmFPh/ZfD4O2AU/D5eEPnXJgD4ZVQY/tr+DPnkjgz7VzAY/5+OCPt16hT51Pwc/xQOCPl/Phz73rAc/kh+BPv8g"
        "ij6QFQg/tTeAPr1vjD5weQg/mph+Ppm7jj6p2Ag/Brx8PnEEkT5uMwk/8dl6PiNKkz7fiQk/nfJ4PhWNlT4v3Ak/1QZ3PuLMlz5eKgo/Hhd1PqsJmj7BdAo/"
        "vCNzPnBDnD5Wuwo/ui1xPlN6nj5h/go/oDVvPhCuoD7zPQs/8zttPsreoj4+egs/s0BrPoAMpT5jsws/7URpPlQ3pz6F6Qs/oUhnPkZfqT7FHAw/mExlPlWE"
        "qz40TQw/FlFjPoOmrT4Deww/n1ZhPu/Frz5Vpgw/eV1fPpvisT5Kzww/J2ZdPmX8sz7k9Qw/73BbPrITtj5lGg0/E35ZPl8ouD7ePA0/GY5XPm06uj5fXQ0/"
        "RaFVPv1JvD4cfA0/2LdTPhFXvj4TmQ0/GNJRPshhwD5XtA0/v+9PPiNqwj4Hzg0/mRFOPmVwxD425g0/YTdMPm10xj4F/Q0/F2FKPlx2yD5zEg4/ho9IPjJ2"
        "yj6RJg4/J8JGPhB0zD6COQ4/PPlEPhlwzj5FSw4/xjRDPk1q0D7ZWw4/CHVBPsxi0j5haw4/fLk/PpZZ1D7deQ4/ZAI+Ps9O1j5dhw4/wk88PpZC2D7ikw4/"
        "UaE6Pso02j5rnw4/z/Y4Pq8l3D4Iqg4/wlA3PkQV3j68sw4/YK41PooD4D6UvA4/qg80PsPw4T5yxA4/4nQyPs/c4z51yw4/QN0wPu/H5T6N0Q4/w0gvPgOy"
        "5z7L1g4/rrctPiyb6T4O2w4/OSksPoyD6z523g4/pp0qPiNr7T7j4A4/bhQpPhFS7z5U4g4/UI0nPlg48T7K4g4/jQgmPvcd8z5D4g4/XoUkPjID9T6g4A4/"
        "wAMjPsXn9j7f3Q4/toMhPhTM+D7x2Q4/PgUgPv+v+j7l1A4/04cePoaT/D6azg4/dAsdPsl2/j4Axw4/ZJAbPuQsAD8Gvg4/YRYaPlQeAT+8sw4/rp0YPqEP"
        "Aj/wpw4/SiYXPu8AAz/Dmg4/NrAVPhvyAz/0iw4/tDsUPkfjBD+Bew4/gsgSPnTUBT9ZaQ4/aVcRPqDFBj9tVQ4/q+gPPru2Bz+rPw4/jXwOPuenCD8CKA4/"
        "lBMNPhOZCT9SDg4/iq4LPlCKCj+Z8g0/vk4KPnx7Cz/Y1A0/7fMIPspsDD/dtA0/Zp8HPgdeDT+Wkg0/9FEGPmZPDj/0bQ0/KA0FPsRADz/2Rg0/idEDPiMy"
        "ED9YHQ0/MKECPpIjET898Qw/5XwBPgEVEj9hwgw/SWcAPoEGEz/mkAw/zsL+PfD3Ez+JXAw/K9r8PXDpFD9bJQw/2xj7PeDaFT8p6ws/iIL5PU/MFj/zrQs/"
        "cRz4Pb69Fz+YbQs/yOr2PR2vGD8XKgs/y/L1PWqgGT8/4wo/Mjn1PaeRGj8xmQo/tcL0PcOCGz+6Swo/DJT0Pb1zHD+5+gk/gbP0PaZkHT8vpgk/wCT1PVxV"
        "Hj8JTgk/B+31PfFFHz858gg/DhH3PUQ2ID+rkgg/FJb4PWMmIT9iLwg/t376PVEWIj8qyAc/NdD8PeoFIz8DXQc/qIz/PUH1Iz/u7QY/mlsBPjLkJD/IegY/"
        "PSkDPuHSJT+CAwY/STAFPhrBJj8aiAU/Q3EHPv+uJz+BCAU/s+wJPl6cKD+lhAQ/mKIMPlmJKT92/AM/NpMPPrx1Kj/0bwM/Br4SPqphKz/83gI/gSIWPgFN"
        "LD+hSQI/ZsAZPrA3LT/RrwE/ZJYdPskhLj9rEQE/saMhPjkLLz9+bgA/huclPvHzLz/Wjf8+TmAqPvDbMD+DNf4+/gwvPibDMT+/0/w+iewzPpOpMj+taPs+"
        "Gv04PhWPMz/p8/k+5j0+Pr1zND+0dfg+Ga1DPnlXNT/u7fY+6UlJPks6Nj90XPU+fxJPPhEcNz9IwfM+0QVVPsr8Nz9pHPI+0SJbPnfcOD/XbfA+MGhhPvW6"
        "OT8tte4+ndRnPmeYOj+u8uw+DmduPop0Oz9bJus+dR51Pn9PPD/wT+k+xvl7PjUpPT+xb+c++nuBPooBPj97heU++guFPpDYPj8ukeM+fqyIPiWuPz/JkuE+"
        "Ql2MPkmCQD8rit8+wR2QPvxUQT91d90+dO2TPhwmQj+nWts+GMyXPqn1Qj/CM9k+SbmbPqTDQz/FAtc+orSfPvyPRD+wx9Q+Ab6jPp9aRT+EgtI+4dSnPo4j"
        "Rj8eM9A+HvmrPqfqRj9e2c0+eCqwPvuvRz+Gdcs+iGi0PmlzSD+WB8k+C7O4PvA0ST+Oj8Y+ngm9PpD0ST9ODcQ+QGzBPimySj84gcE+jNrFPsptSz/q6r4+"
        "P1TKPlInTD+lSrw+ONnOPtPeTD9qoLk+VWnTPhiUTT/267Y+UwTYPjRHTj+MLbQ+zqncPhb4Tj9NZbE+o1nhPr2mTz86k64+kBPmPhpTUD90t6s+UtfqPir9"
        "UD/60ag+paTvPs+kUT8R46U+Z3v0PidKUj906qI+eVv5PgPtUj+K6J8+UkT+PmGNUz9y3Zw++poBP1IrVD8MyZk+DRgEP8XGVD+9q5Y+QpkGP6tfVT9ihZM+"
        "dR4JPwH2VT8/VpA+dqcLP7mJVj/aHo0+MzQOP+MaVz8z34k+esQQP36pVz/Ql4Y+GVgTP3o1WD/USIM+/u4VP8a+WD8A5X8+6IgYP4RFWT89K3k+xCUbP6PJ"
        "WT+hZHI+YcUdPyNLWj/Akms+e2cgPwTKWj+mtmQ+AgwjP1ZGWz+i0V0+orIlPxrAWz/N5VY+OlsoP1A3XD+69E8+lgUrP/erXD8IAUk+dbEtPzIeXT8TDUI+"
        "ol4wPwCOXT9DHDs+3QwzP2H7XT++MTQ+4Ls1P3dmXj+1US0+i2s4P0LPXj9ngSY+ixs7P+M1Xz8Rxh8+m8s9P1uaXz+FJhk+eHtAP8r8Xz9cqhI+4CpDP1Nd"
        "YD+BWgw+odlFP/W7YD9wQQY+VYdIP9IYYT8ragA+2zNLPx10YT8uxfU9395NP8TNYT/Fcus9DohQPwsmYj+c/eE9RS9TPwN9Yj9MiNk9QdRVP8zSYj8RONI9"
        "sHZYP4knYz+QMMw9XRZbP1t7Yz/qlMc9B7NdP2TOYz8Cg8Q9jExgP8UgZD9vEsM9qOJiP59yZD9yU8M9OnVlPwXEZD9JS8U9/wNoPzgVZT/D9cg91o5qPzhm"
        "ZT+3RM49SBVtP2u3ZT8tI9U9aJdvP68IZj/Jc909MxVyP0daZj+cF+c9io50PzKsZj8Y7fE9SwN3P6T+Zj/H1P09ZHN5P61RZz8VVwU+xt57P12lZz+6Lgw+"
        "gEV+P+j5Zz/1YxM+"
    ),
    "magma": (
        "lKC/OnZR9Dk4LmM89PoTO/28qTrlKpY8fuRWO3wPFztIN8I8ZtmTO3y4ZDspefU8OPjCOweynjugFRg9wqT4O/5F0DucNTg9gm8aPLVuAzzzclg9stc7PJ8F"
        "ITz+1Hg9hZdgPCfbQDxJoYw9llmEPCvBYjwJ4pw96iGaPPVIgzxgOq09bLOxPNMTljxQqr09mBjLPIGyqTw4L849NWLmPAYQvjy4y949qtMBPR8R0zxZi+89"
        "a30RPdOg6DzKNgA+ADwiPXWw/jwouAg+FoczPVORCj2QShE+qdxEPTnxFT1S7xk+f01WPTxpIT03pyI+IeVnPfevLD33dis+qaV5Pep5Nz0pWzQ+vMuFPYXQ"
        "QT1UVD0+buCOPX2tSz14YkY+DhSYPccPVT0ahk8+wmmhPQvwXT08v1g+veWqPTBMZj2ZDWI+nIq0Pd4cbj2scGs+DFy+PeZddT1o53Q+q1zIPe4HfD3BcH4+"
        "rJDSPWMLgT1xBYQ+J/rcPRLCgz0b2og+1J3nPasghj2ito0+Un7yPSQmiD2rmJI+KJz9PfbRiT10fZc+MXwEPoEhiz0GY5w+VUsKPpUQjD2uR6E+FD0QPnia"
        "jD3YKaY+z04WPoLGjD19A6s+1IEcPo6RjD2m0q8+ndUiPi/9iz2Gk7Q+gEYpPuwUiz3yP7k+iNUvPjTXiT2y1b0+NX02Pv9YiD1uTcI+eTw9PoCehj1mpMY+"
        "Fw5EPk2/hD1v1Mo+6e5KPhXKgj1F2s4+e9pRPmPVgD33sdI+msxYPlPrfT3mWNY+nMFfPtCAej37zNk+kbVmPi2Vdz1KDd0+mKVtPitOdT2PGeA+zo50PhnI"
        "cz1z8uI+oG97PhUbcz1nmeU++yKBPiVdcz0fEOg+6IiEPkeOdD33WOo+q+iHPhO7dj1Lduw+zEKLPtjUeT39au4+opaOPqXcfT2sOfA+GeWRPjlegT0Z5fE+"
        "7S2VPl00hD3Bb/M+YXGYPlpohz1E3PQ+gbCbPhTtij3+LPY+ZOqePuy/jj0oZPc+eSCiPjXSkj26g/g+BVOlPgQblz2Ljfk+oYGoPjWXmz3Tg/o+fa2rPjI6"
        "oD1/Z/s+u9auPr3+pD0hOvw+Wf2xPpjfqT1t/fw+vCG1PgrYrj1Psv0+jUS4Pr3gsz2wWf4+7WW7Poz2uD2d9P4+/YW+PlEWvj3gg/8+36TBPmw9wz1kBAA/"
        "18LEPjRoyD2rQQA/aeDHPoGTzT0pegA/uf3KPkm+0j0yrgA/xRrOPnHm1z3o3QA/0jfRPmcK3T2NCQE/vVTUPqYp4j2HMQE/63HXPppC5z3FVQE/n4/aPjdU"
        "7D15dgE/2q3dPvZd8T20kwE/vMzgPsxe9j2XrQE/aOzjPrhW+z1ExAE//gznPpoiAD661wE/fy7qPiGVAj4d6AE/7FDtPqwCBT579QE/p3TwPjxrBz7F/wE/"
        "cJnzPo7OCT4cBwI/Zr/2PigtDD6RCwI/rOb5PsaGDj4CDQI/Yg/9PmrbED6ACwI/tBwAPxMrEz4MBwI/cLIBPwR2FT6T/wE/5EgDPzy8Fz449QE/IuAEPwD+"
        "GT7J5wE/GHgGPww7HD5W1wE/2BAIP+dzHj7fwwE/UKoJP9KoID5UrQE/kUQLP4zZIj6jkwE/nN8MP5oGJT7NdgE/cHsOP/0vJz7BVgE//BcQPztWKT5/MwE/"
        "QrURPxB5Kz4GDQE/UFMTP0aZLT4m4wA/F/IUP922Lz7+tQA/hpEWP9TRMT5ehQA/rTEYP/fqMz5VUQA/fNIZP0MCNj7SGQA/83MbP/wXOD5qvf8+ARYdP6os"
        "Oj4cQP8+prgeP45APD53u/4+0VsgP+tTPj57L/4+gv8hPwZnQD4onP0+qaMjP6d6Qj47Af0+NEglPxGPRD6zXvw+JO0mP0SkRj5wtPs+WJIoP027SD5xAvs+"
        "3zcqPyzUSj62SPo+h90rP6rvTD79hvk+YoMtP04OTz5Fvfg+TikvP1kwUT6O6/c+Kc8wP1RWUz7YEfc+BHUyP0mBVT4BMPY+rBo0P32xVz7pRfU+EsA1P3Xn"
        "WT6xU/Q+I2U3Pz4kXD42WfM+wAk5PxtoXj56VvI+5q06Pxi0YD57S/E+VVE8P7wIYz5cOPA++fM9P89mZT78HO8+s5U/P1/PZz57+e0+cjZBPzVDaj77zew+"
        "8dVCP13DbD5bmus+MnREP11Qbz7dXuo+4BBGP0LrcT6kG+k+/KtHP1uVdD7Q0Oc+MUVJP3JPdz6EfuY+f9xKP5Maej5bJOU+k3FMPw74fD4ew+M+OgROP6vo"
        "fz4xW+I+MZRPP/92gT6W7OA+RyFRP6sEgz7Rd98+R6tSP7+dhD5I/d0+3zFUP+FChj5ffdw+3bRVP9z0hz6x99o+7DNXPzW0iT7Sbdk+uK5YP5WBiz4F4Nc+"
        "7iRaP8RdjT4zT9Y+W5ZbP2tJjz7ku9Q+igJdP+1EkT58JtM+OGlePxZRkz4qkNE+AMpfP4tulT4a+s8+jSRhP7Kdlz58Zc4+fXhiPxHfmT720sw+acVjP1Ez"
        "nD7ZQ8s+DwtlP5Ganj62uck+CklmP1kVoT4ANsg+9n5nP+yjoz7lucY+n6xoP0pGpj4XR8U+kdFpP5P8qD5M38M+q+1qP6jGqz44hMI+lwBsP2akrj5tN8E+"
        "NQptP4mVsT6g+r8+UgpuP42ZtD6Fz74+zgBvP+qvtz6Nt70+t+1vP/nXuj7QtLw+3dBwPxIRvj47yLs+YapxP2xawT4b87o+Y3pyP/uyxD4EN7o+9kBzP48Z"
        "yD5olbk+TP5zP2GNyz5nDrk+hbJ0P4QNzz4Oo7g+5l11Pw+Z0j7BU7g+wQB2P28u1j5sIbg+fJt2P7jM2T5SDLg+OC53PyFz3T4vFLg+Sbl3P8Ag4T4EObg+"
        "8zx4P8zU5D6verg+mbl4PzeO6D7t2Lg+fy95P1lM7D56U7k++Z55P40O8D6v6bk+Wwh6P+XT8z5Km7o++Gt6P/6b9z6hZ7s+BMp6PzBm+z4OTrw+0SJ7P/Qx"
        "/z7GTb0+o3Z7P3N/AT9FZr4+rMV7P1FmAz/hlr8+MBB8P3JNBT+P3sA+YFZ8P7U0Bz/qPMI+X5h8P+cbCT8HscM+XtZ8PwgDCz8/OsU+gBB9PwfqDD/H18Y+"
        "5UZ9P8TQDj8aicg+r3l9Pz23ED9uTco+ual9P9ycEj8+JMw+v9Z9P+SBFD+/DM4+jwB+P4hmFj9sBtA+KCd+P8dKGD+dENI+nUp+P7IuGj/tKtQ+6Gt+P6ER"
        "HD9xVNY+CYt+P6XzHT/njNg+Jqd+P2fVHz/I09o+UcB+P9S2IT+uKN0+x9d+P0aXIz/0it8+Z+1+P812JT8S+uE+JgB/PzJWJz8IduQ+NBB/P0Q1KT9y/uY+"
        "3h9/P9MSKz//kek+pSx/P0HwLD9ZMew+ejZ/P9HNLj9/3O4+cEB/P5upMD82kfE+lUd/P3eFMj8zUfQ+Ckx/P2NhND/vG/c+sVB/P6w7Nj9S7/k+ZVJ/PzcW"
        "OD91zfw+ZVJ/P1/wOT8Htf8+vVF/P5vJOz+gUgE/Ek5/PzyjPT/IzwI/Vkp/P697Pz/fUAQ/cER/PyJUQT+d1gU/ozx/P4QsQz/QYAc/tTR/P+oDRT+v7gg/"
        "gCl/PwrcRj+IgQo/Rx9/P7eySD92Fww/ChJ/P+yJSj8csg0/eQR/P4lgTD9dUA8/ZvV+PwQ3Tj+d8hA/4uR+P4ANUD/dmBI/G9R+P1TjUT+FQhQ/6MB+P665"
        "Uz+A8BU/jq5+P/yOVT9uoRc/IJl+PyNlVz/zVhk/VYV+P+s5WT/lDhs/AW5+P+APWz+fyxw/91h+P1TkXD9hih4/ZEB+P+W5Xj/sTSA/LCp+PxWOYD9uEyI/"
        "jBB+P3NjYj+H3SM/i/l9P2E3ZD9lqSU/RN99P2sMZj/IeSc/78d9PxXgZz+MSyk/l619P8y0aT+SISs//5V9P1WIaz8J+Sw/HHx9P7hcbT891C4/hGR9Py8w"
        "bz/RsDA/jEt9Py4EcT+bkDI/JjR9P7bXcj/ncTQ/jxx9P4KrdD9+VTY/nwV9Pyx/dj/rOjg/u+98P7VSeD+4ITo/Udl8P8Qmej+NCjw/ZcV8P0z6ez/Y8z0/"
        "ga98P+HOfT9/3z8/"
    ),
    "inferno": (
        "lKC/OnZR9Dk4LmM885EUOyF2pjodIJg8CTRYO/VjEzvekMY8AP+UO1FMXjvfNP08+83EO1m/mTv+7h099Ib7O4AQyTsb1z89vqUcPFW9/Dug3WE9KxY/PMNJ"
        "GjxR94E9SUtlPBDpNzxiLJM976qHPGE4VzzkaqQ9ILSePGfwdzx5y7U9xeK3POvkjDxhU8c910vTPAxcnjzU8dg9YRvxPA8nsDxqvuo9tr4IPbIqwjyRt/w9"
        "w0kaPUdY1DzTZwc+exEtPcOD5jxEhxA+8SlAPQpq+DyXxBk+qYhTPXUDBT17EyM+ETdnPTmYDT24dCw+pz97PWXfFT3J5zU+jNiHPV+2HT33cj8+XkmSPVIL"
        "JT0GEUk+3POcPZSkKz35vFI+sdunPbN4MT24dFw+igSzPVqANj1hNWY+i3G+PT21Oj2L+28+RiTKPQYQPj34wXk+1h7WPXaLQD2UwYE+s2DiPXQlQj1nnIY+"
        "V+nuPfTcQj2obYs+Mbf7PRy1Qj0FMZA+SWMEPk62QT0q4pQ+YwkLPhTsPz09fJk+issRPkBoPT2p+p0+mKYYPqc8Oj33WKI+JJcfPn+DNj20kqY+8pcmPq5l"
        "Mj1Io6o+EqUtPvIILj0Jh64+lbo0PiWVKT2bO7I+0NQ7PgYwJT3CvrU+ke9CPnkCIT2VD7k+OghKPlJJHT2MLbw+KhxRPgMkGj0NGb8+SilYPsWsFz0C08E+"
        "Bi5fPpz5FT3/XMQ+RihmPmkdFT3YuMY+TBhtPmkdFT2n6Mg+1v1zPuf/FT3I7so+odh6PvzGFz24zcw+VtSAPo9wGj2Qh84+PzeEPqD8HT3NHtA+LZWHPuVk"
        "Ij2rldE+/u2KPtSdJz2F7tI+W0KOPld6LT0wK9Q+hpKRPhfzMz2lTdU+496UPjT1Oj2XV9Y+tyeYPudvQj2ZStc+RG2bPnZTSj09KNg+za+ePiWQUj318dg+"
        "t++hPlUYWz3OqNk+Iy2lPnrgYz0WTto+VWioPgHcbD254to+kKGrPnkBdj1/Z9s+F9muPoBIfz2Y3ds+Cg+yPmVVhD1nRdw+r0O1PvkPiT22n9w+JXe4Pl/R"
        "jT0t7dw+sKm7PgOYkj1RLt0+c9u+Pr9glz2IY90+awzCPogqnD1Yjd0+mzzFPlH0oD1HrN0+h2zIPg69pT12wN0+7ZvLPqWCqj0qyt0+MsvOPpFErz2jyd0+"
        "VfrRPtECtD0Fv90+VinVPlq8uD20qt0+WFjYPipxvT2wjN0+e4fbPkIhwj0bZd0+nrbePh3Mxj03NN0+4uXhPrlxyz3k+dw+SBXlPhcS0D2Fttw+8kToPkOu"
        "1D08atw+vHTrPjFF2T3GFNw+qaTuPu3X3T1Gtts++tTxPndm4j2YTts+jgX1PtDw5j0B3to+RDb4Pn136z2AZNo+PGf7Pov77z304dk+eJj+Pvp89D1+Vtk+"
        "6+QAP1D8+D0ewtg+qn0CP5p6/T3VJNg+ahYEP6n7AD6Aftc+S68FP8E5Az4gz9Y+G0gHPxx4BT61FtY+/OAIP/62Bz5hVdU+vHkKP2b2CT4Ai9Q+exIMPx43"
        "DD63t9M+GasNPyV5Dj5A29I+hUMPPwG9ED6+9dE+z9sQPzoDEz4xB9E+53MSP89LFT6ZD9A+uwsUP4mXFz71Ds8+K6MVP6zmGT5oBc4+WDoXP3o5HD7Q8sw+"
        "D9EYP3mQHj4K18s+UWcaPzHsID46sso+Df0bPydNIz5/hMk+Q5IdP1uzJT7bTcg+wCYfP9ofKD5ODsc+lbogP6OSKj74xcU+sU0iPz0MLT7adMQ+498jP3GN"
        "Lz70GsM+THElP4MWMj5FuME+qAEnP7WnND7PTMA+CJEoP9FBNz7T2L4+Sx8qP1zlOT50XL0+YKwrP5uSPD6Q17s+JjgtP1ZKPz5rSro+i8IuP40MQj4ktbg+"
        "kEswP03aRD6+F7c+E9MxP5azRz5YcrU+81gzP3SZSj4VxbM+L900P6SLTT7UD7I+ll82PzOLUD74UrA+JuA3P2OYUz6Cjq4+0F45P7yzVj7Xwqw+Uds6P3/d"
        "WT7U76o+uVU8P3YWXT7fFak+5s09P+VeYD74NKc+t0M/Pw+3Yz5iTaU+HLdAP3kfZz4cX6M+8idCP2eYaj6MaqE+KZZDP6Mibj6xb58+nwFFPyu+cT6tbp0+"
        "RGpGP0RrdT7DZ5s+9s9HP7cqeT4UW5k+pTJJP0D8fD7DSJc+LpJKPzNwgD4SMZU+cO5LP7Vrgj5EFJM+a0dNP+twhD5a8pA+7ZxOP5F/hj64y44+5e5PPy2Y"
        "iD5eoIw+Qz1RP3y6ij6PcIo+5IdSP5/mjD5LPIg+p85TP9ocjz4ZBIY+jBFVPwtdkT60x4M+clBWPzOnkz6lh4E+SItXP1D7lT6Qh34+7MFYP6dZmD7C+Hk+"
        "TfRZP9PBmj4kY3U+SyJbPxY0nT61xnA+5EtcP0+wnz77I2w+CXFdP342oj72emc+l5FeP4LGpD4tzGI+fa1fPzlgpz5dF14+rMRgP8UDqj7IXFk+E9dhP+Kw"
        "rD5vnFQ+sORiP29nrz7Y1k8+Y+1jP2snsj58C0s+LPFkP7fwtD7iOkY+6e9lPy/Dtz6EZEE+q+lmP7Keuj7oiDw+QN5nP/2CvT6Hpzc+yM1oPzNwwD6lwDI+"
        "JLhpP8tlwz5B1C0+QZ1qP+ljxj7W4Sg+MX1rP0hqyT5k6SM+0VdsP8h4zD7q6h4+Iy1tPyaPzz4l5hk+Jv1tP2Ct0j4W2xQ+2sduPzXT1T55yQ8+Ho1vP2AA"
        "2T7JsAo+AU1wP+M03D6KkQU+hQdxP3pw3z44awA+qbxxPwOz4j4ofPY9TGxyP1385T66E+w9fxZzP0RM6T6qneE9MLtzP5ii7D5+Gtc9gVp0Pzf/7z69isw9"
        "QfR0P91h8z5078E9f4h1P4rK9j5AS7c9TBd2P/w4+j62n6w9iKB2PzKt/T4G8aE9QiR3P2STAD9jQ5c9aqJ3P/BSAj8XnYw9ERt4PwkVBD//BYI9Jo54P7LZ"
        "BT88Em89qft4P9egBz9Ealo9mWN5P2pqCT+xNkY9+MV5P1k2Cz/KqDI9tCJ6P4EEDT/l8h893Xl6P/bUDj/PEw89ZMt6P5OnED+5pgA9SBd7P0p8Ej+ciek8"
        "eV17PwlTFD89Ctc8F557P9ArFj/eBco88dh7P30GGD9OucI8KA58PyLjGT9fYcE8mz18P4vBGz9GQ8Y8Wmd8P8uhHT9QptE8ZYt8P8+DHz8w2uM8rKl8P3dn"
        "IT/GMv08HsJ8P8JMIz8UBA89zNR8P7EzJT+BXyM9teF8PyIcJz8lszo9uOh8PyUGKT/P91M99+l8P4jxKj9k6m49T+V8P0zeLD92pYU909p8P3HMLj8ddZQ9"
        "ccp8P9S7MD/M0aM9KbR8P3WsMj9PrLM9+pd8P0WeND83+8M993V8PzKRNj8gttQ9Dk58PyuFOD9R2OU9HSB8PzF6Oj8gXvc9V+x7PzNwPD+6ogQ+vLJ7P+1m"
        "Pj+gxg0+S3N7P4FeQD9IGxc+Jy57P6xWQj+yoCA+YeN6P25PRD9xWCo+CJN6P5VIRj8LQzQ+Pj16Pw9CSD+ZYj4+N+J5P7w7Sj/xuEg+4IF5P4s1TD+ySFM+"
        "TBx5P0kvTj8BFV4+ILJ4P8MoUD8uH2k+s0N4P5YhUj8aanQ+idF3P48ZVD+p+H8+tFt3P50QVj/J54U+huJ2P2wGWD/o+Ys+hGd2P1X6WT8WM5I+lut1P/Lr"
        "Wz/ElJg+rW51PxLbXT/NI58+E/N0P+vGXz/s36U+r3p0P4KuYT+Gyaw+5gV0P7SRYz+j5rM+hZhzPxFvZT92M7s+YTRzP9BFZz/hssI+5NxyP8IUaT9SY8o+"
        "hZVyP6naaj+vQtI+E2JyP0aWbD+QTdo+v0ZyP1pGbj/tfeI+eEdyP6fpbz+SzOo+PGhyP0F/cT9FL/M+AKxyP4EGcz8wnPs+YhVzPwJ/dD8dAwI/PKVzPwjp"
        "dT8rMgY/A1x0P/ZEdz8ZVQo/rDh1P6eTeD8KaA4/UDl2PyjWeT+taRI/GFx3P7cNez8iUxY/E554P3E7fD/EJho/oPx5P3RgfT/84x0/MnV7P+19fj9ViiE/"
        "SwV9P8iUfz+9GSU/"
    ),
    "plasma": (
        "aF5OPWwl9DxfKQc/Kh+CPaXd6DzRegg/rFKaPR7f3jzUugk/KZWwPRkE1jyi6wo/WmLFPdUmzjzxDgw/CwzZPasjxzx0Jg0/IsbrPYP4wDwnMw4/28D9PaVq"
        "uzxZNg8/444HPmlWtjwnMRA/PPoPPu+osTw6JBE/bywYPidLrTxaEBI/1CwgPkksqTzt9RI/9wEoPqc9pTyZ1RM/GLEvPnpuoTy0rxQ/qz43Pl+2nTyQhBU/"
        "n64+PsAImjyTVBY/1QNGPiFbljzeHxc/dEFNPjenkjy05hc/12lUPobijjxIqRg/kX5bPvYKizy6Zxk/d4FiPrckhzwdIho/YHRpPh0hgzyQ2Bo/IVlwPhr8"
        "fTwmixs/gzB3PntqdTzvORw/Gvx9Po6RbDzr5Bw/eF6CPlRxYzwZjB0/x7mFPswJWjxqLx4/XhCJPsVWUDz/zh4/w2KMPtRkRjy2ah8/GLGPPio4PDx+AiA/"
        "oPuSPivZMTxoliA/wEKWPm1UJzxCJiE/mIaZPr6lHDwcsiE/j8ecPrLZETzFOSI/owWgPt/8Bjw8vSI/GEGjPhhA+DtgPCM/EHqmPjmX4jsPtyM/q7CpPhMp"
        "zTtJLSQ/yeSsPjMXuDvcniQ/8BawPouLozu3CyU/3EazPuGWjzvJcyU/sHS2Pt7neDvg1iU/jKC5PoOIVDvsNCY/ksq8PiOFMjvKjSY/gPK/PtogEztY4SY/"
        "mBjDPr3D7Tp3Lyc/2jzGPg71uzoleCc/JF/JPqMDkjofuyc/mX/MPoQuYTpV+Cc/F57PPs+7MTqlLyg/nbrSPtFBFzr+YCg/LNXVPmbZEzo/jCg/xO3YPlNY"
        "KTpXsSg/IQTcPnfXWToU0Cg/hxjfPti3kzp16Cg/siriPtPZyTpI+ig/xTrlPpxQCDt9BSk/WkjoPjuNNDsTCik/tVPrPsU5ajvqByk/klzuPjnulDvf/ig/"
        "0GLxPoQOujsD7yg/b2b0Pny45Ds02Cg/TWf3PtCbCjxzuig/a2X6PrfrJTyvlSg/hWD9PrRxRDzXaSg/bywAP/FGZjzrNig/+KYBP8nMhTzb/Cc/7x8DP6pH"
        "mjzHuyc/QpcEP+OksDywcyc/0AwGP1X3yDyFJCc/mYAHP61N4zxXziY/nfIIP8u6/zw3cSY/zGIKP7snDz1FDSY/8tALPzuOHz1zoiU/Mj0NP2CvMD3gMCU/"
        "eqcOPyfeQT2uuCQ/mQ8QP9ogUz3vOSQ/n3URP3l3ZD3EtCM/jNkSP+zfdT1OKSM/PzsUP5+tgz2elyI/ppoVPyZzjD34/yE/0/cWPxBBlT1rYiE/pFIYP8oV"
        "nj0rvyA/CKsZP9zxpj1qFiA/EQEbPznUrz1aaB8/rFQcP+C8uD0ctR4/26UdP8WqwT3j/B0/jPQeP+mdyj3yPx0/r0AgPz6V0z18fhw/VYohP0uR3D2yuBs/"
        "bNEiP36Q5T237ho/5BUkP1yT7j3vIBo/3lclP1+Z9z1ZTxk/SpcmPwFRAD5behg/F9QnP6HWBD4Wohc/RQ4pPwtdCT7OxhY/5UUqPz/kDT606BU/9norP39s"
        "Ej4LCBU/ea0sPwL1Fj7mJBQ/bt0tPwt+Gz6WPxM/xAovP1cHID5PWBI/nDUwP+aQJD4zbxE/9l0xP7kaKT6EhBA/04MyP4ukLT5jmA8/IqczP14uMj7zqg4/"
        "Fcg0PzC4Nj53vA0/iuY1P8BBOz4QzQw/kwI3P0/LPz7P3As/Pxw4P5tURD726wo/oDM5P6XdSD6p+gk/lUg6P2tmTT72CAk/T1s7P+7uUT4BFwg/vms8Py13"
        "Vj77JAc/A3o9Pyr/Wj4FMwY//YU+P+SGXz4QQQU/3o8/P1oOZD48TwQ/hZdAP46VaD68XQM/JJ1BP8EcbT5/bAI/qaBCP7GjcT63ewE/J6JDP14qdj5UiwA/"
        "jKFEP0+xej7ONv8+Cp9FP/w3fz4hWP0+kZpGP3bfgT7Eevs+IZRHP80ihD62nvk+yotIP2Zmhj4axPc+jIFJPwCqiD7N6vU+eXVKP7vtij7PEvQ+kGdLP7ox"
        "jT5kPPI+4ldMP/t1jz5JZ/A+X0ZNP4C6kT7Ak+4+FjNOP0f/kz6pwew+CB5PP3RElj4C8eo+VwdQPwWKmD4QIuk+0O5QP/rPmj5tVOc+ptRRP3YWnT5diOU+"
        "x7hSP5pdnz6dveM+RZtTP0SloT4s9OE+D3xUP5btoz4KLOA+JVtVP482pj44Zd4+lzhWP3OAqD6Vn9w+ZhRXP//Kqj5i29o+ke5XP3YWrT47GNk+GcdYP9hi"
        "rz4hVtc+7Z1ZP0ewsT4UldU+HXNaP8H+sz7x1NM+qkZbP0hOtj66FdI+kxhcP/6euD5tV9A+yehcP+Hwuj4Lms4+SrddPxNEvT5R3cw+FoReP7eYvz4+Ics+"
        "QE9fP6ruwT7UZck+pBhgPw9GxD7vqsc+VOBgPwafxj5v8MU+QKZhP5D5yD6XNsQ+ZmpiP85Vyz4DfcI+xyxjP8CzzT7Sw8A+Uu1jP2YT0D7lCr8+CKxkP+J0"
        "0j47Ur0+12hlPzTY1D6zmbs+0SNmP5891z5M4bk+09xmPwGl2T4HKbg+7pNnP1oO3D7BcLY+E0loP+553j58uLQ+L/xoP7zn4D4VALM+Q61pP8VX4z7QR7E+"
        "T1xqPwjK5T5Hj68+MQlrP6c+6D6/1q0+6rNrP6K16j7zHaw+iVxsPzwv7T7lZKo+3gJtPzKr7z60q6g++KZtP8cp8j5B8qY+x0huP/yq9D6LOKU+S+huP/Eu"
        "9z6RfqM+c4VvP2O1+T52xKE+HSBwP9k+/D7VCaA+WrhwP+/K/j4ST54+Gk5xP/OsAD/qk5w+TOFxP+D1AT+A2Jo+73FyPz5AAz/zHJk+4/9yPx6MBD8CYZc+"
        "SItzP3/ZBT8SpZU+2xN0P2MoBz956JM+r5l0P8h4CD+/K5I+sBx1P8HKCT/jbpA+0Jx1P0seCz/msY4+Hhp2P2lzDD/H9Iw+eZR2PxnKDT+oN4s+0At3P1si"
        "Dz+Jeok+E4B3P0J8ED+MvYc+UvF3P9zXET9LAIY+W194Pwk1Ez8tQ4Q+Lsp4P+qTFD9RhoI+yjF5P2/0FT/ayYA+IJZ5P5dWFz9MG34+L/d5P3O6GD8zpHo+"
        "xVR6PwQgGj8nLnc+BK96PziHGz+uuXM+uAV7PyDwHD8LR3A+81h7P7xaHj+A1mw+k6h7Pw3HHz9RaGk+d/R7PzM1IT87/GU+sDx8P/2kIj9Lk2I+G4F8P4sW"
        "JD/DLV8+ysF8P76JJT+vzFs+m/58P8X+Jj/Ob1g+fjd9P4J1KD8rGFU+YWx9P/LtKT+PxlE+RZ19PydoKz8+e04+Gcp9PxHkLD9DN0s+u/J9P79hLj9q+0c+"
        "Kxd+PzPhLz82yEQ+WDd+P1piMT88n0E+IlN+PzblMj+IgT4+mGp+P+hpND+gbzs+iX1+P07wNT9Zazg+BYx+P2h4Nz8EdjU+2ZV+P0cCOT/vkDI+B5t+P+uN"
        "Oj+tvS8+jZt+P0MbPD8V/iw+OZd+P1CqPT+5Uyo+DY5+PxA7Pz+xwCc+BoB+P5bNQD8XRyU+BW1+P79hQj8D6SI+1lR+P773Qz8JqCA+aTd+P3GPRT/9hR4+"
        "zxR+P9goRz8Fhhw+9ux9P+PDSD/Bqho+3799P6JgSj9J9hg+aY19P/T+Sz88axc+k1V9P9ieTT+zCxY+CRh9P5JATz932BQ+u9R8P+/jUD/l0xM+24t8P9+I"
        "Uj+bABM+ij18P0AvVD8tYBI+del7PzTXVT/c8hE+Jo97P/6AVz/htxE+RS97PxcsWT+WsRE+88l6P4DYWj8z3xE+4V16P8+GXD9DPBI+gex5P0w2Xj+byhI+"
        "GXV5PzrnXz+6hBM+uvd4P5qZYT+yZhQ+2nR4PydNYz/KaxU+4et3PyUCZT/XihY+iV13P0G4Zj9/vBc+Fcp2P2lvaD9z9Bg+ujB2P/Inaj/qIRo+HZN1P1Th"
        "az8eNBs+XvF0P1+bbT8bERw+J0x0PyFWbz9Tlxw+UaRzP1oRcT9fmBw+j/tyP6PMcj+N1Bs+glRyP1WHdD+V7xk+8rNxPyFAdj+7YhY+GSBxP4T1dz/FVhA+"
        "06RwP/SjeT9TegY+"
    ),
    "cividis": (
        "AAAAAM1aCj5TCJw+AAAAALNhDT4oSZ8+AAAAALZlED63maI+AAAAAORnEz744KU+AAAAAO1mFj6LNKk+AAAAANBiGT7Jk6w+AAAAAFBWHD74+a8+AAAAACYb"
        "Hz68dLM+AAAAAO24IT7+DLc+AAAAAM1YJD4zpLo+AAAAAK34Jj5nQ74+AAAAAI2YKT4D7sE+AAAAAKs9LD7ylMU+AAAAADLmLj5nRMk+AAAAAAOVMT4S+8w+"
        "AAAAANdOND7vrdA+AAAAAN8XNz7yW9Q+AAAAAPn3OT7n/dc+AAAAAK36PD7wi9s+AAAAAKVmPz4N/t4+AAAAAKlMQT5nDuE+AAAAAGaIQz7l1eE+AAAAAL0B"
        "Rj5JFOI+iA9sO+WcSD6tFOI+XD6SPO1KSz5C6+E+xoUDPRwHTj6SruE+dEE9PfPLUD5fYeE+xR1vPY2WUz41CuE+GD+NPZ1lVj6nsuA+nwWhPYI2WT5MT+A+"
        "2iCzPT4JXD5K698+h+HDPc7dXj4eid8+58PTPRyyYT7eH98+qaDiPa2GZD4awd4+j97wPYFbZz6eXd4+SIz+PYwvaj7f+d0+GM4FPlMDbT40nd0+Kh0MPlLW"
        "bz6BQt0+y0cSPsqocj784Nw+jzQYPjV6dT6Hi9w+mPYdPl5LeD6wONw+DJEjPjcbez4Y69s+YhMpPonqfT7Umds+YHMuPqtcgD5qTds+p7MzPmnDgT5KB9s+"
        "x9U4PgYqgz7vxto+ZOc9PmCQhD71g9o+yt5CPjT2hT7LR9o+Br1HPsRbhz62Eto+745MPjPBiD6+2tk+TUpRPj4mij4dqtk+s/BVPiaLiz6RgNk+qI1aPqrv"
        "jD5xVdk+ehdfPg1Ujj6HMdk+LZljPiy4jz5BC9k+TgloPkwckT5T7Ng+c2lsPiiAkj671Ng+TMNwPuPjkz5Nu9g+NA51Pp1HlT5Yqdg+IlR5PhWrlj5Kldg+"
        "Kox9Po0OmD6UiNg+jNuAPgRymT7Pgtg+LO+CPlrVmj4Ue9g+pPyEPrA4nD6Netg+qwiHPgacnT7Nd9g+Dw+JPlz/nj7+e9g+RBSLPrJioD4Xftg+ChCNPirG"
        "oT60kNg+9Q6PPqIpoz6Fl9g+1QSRPjuNpD4dr9g+L/qSPtTwpT5ZxNg+v+6UPm1Upz4419g+296WPkq4qD5O8dg+o8qYPkccqj79Etk+5bWaPkWAqz5yMtk+"
        "F52cPobkrD6jWdk+BoSePsdIrj4Tftk+J2egPm2trz5Uqdk+F0aiPjQSsT613Nk+ByWkPh13sj4fDto+GQSmPifcsz5xPdo+O9+nPpZBtT5+dNo+9rapPian"
        "tj6esto+sI6rPvoMuD4L79o+jGatPhFzuT7DKds+3jqvPknZuj4WbNs+yAuxPgdAvD6Jtts+09yyPuemvT6s/9s+Q660PukNvz6VRtw+bHy2PnF1wD7VlNw+"
        "6Ua4PjzdwT6z7dw+mBW6PkpFwz7vON0+Vd27Pt6txD5wl90+AKm9PnIWxj5G6t0+uW2/Pq5/xz6kUN4+xjbBPi3pyD7nqd4+JvzCPvBSyj7pDd8+xr7EPji9"
        "yz6ned8+RYHGPsQnzT5x5t8+8kTIPtWSzj4eTuA+0QTKPir+zz7GwuA+esXLPuRp0T7CM+E+qYbNPiTW0j57pOE+kUTPPshC1D7mHuI+AAPRPtGv1T6JmOI+"
        "J77SPj8d1z6GHOM+1XnUPjOL2D66n+M+TDbWPq352T5xIOQ+W+/XPmpo2z4AruQ+VKnZPs/X3D7jN+U+X1/bPplH3j6B0eU+HhfdPum33z4KZOY+V87ePp4o"
        "4T4J++Y+mYPgPtmZ4j49mec+7DTiPrsL5D7+Reg+cOrjPuF95T6w5ug+2JrlPmvw5j5vm+k+9UznPuBj6D4wSOo+Mv/oPvHW6T7n/uo+867qPmZK6z4Fwes+"
        "71jsPlnA7D4zh+w+iA3uPhE07j4cQu0+/b7vPpOo7z5sCO4+lGjxPqsh8T5Yxu4+jxrzPhya8j7ic+8+zNT0PuQR9D50DPA+KZf2PpiK9T5NhfA+Z2T4PtED"
        "9z4s1vA+fjb6Ppp7+D72J/E+3Qv8Phf1+T5KYvE+T+j9PlBu+z5ZifE+SMX/PlPo/D4urvE+u9AAP0Fj/j720fE++MEBP1He/z6b4vE+wLICPzatAD8T8vE+"
        "UaQDP3ZrAT/f/fE+aJYEPwsqAj+nBvI+ZYoFP/PoAj+9/fE+NX0GPy+oAz9+API+LnIHP65nBD8o8fE+e2cIP5EnBT+L3vE+ilsJP7jnBT8f2PE+j1EKP0So"
        "Bj9Zv/E+G0gLPyNpBz8Ko/E+Pj8MP0UqCD8wg/E+cjYNP93rCD90YPE+PC4OP7itCT8uOvE+fCYPP/hvCj+AEPE+7x4QP5wyCz/O4/A+8BkRP4T1Cz9EovA+"
        "TRMSP9C4DD9+bvA+/gwTP5F8DT9QN/A+RgcUP5ZADj+Y/O8+pwMVP/8EDz8qre8+l/4VP97JDz+ga+8+DfoWPwCPED9sJu8+nfcXP5dUET8dzO4+uvMYP5Ma"
        "Ej8XgO4+VvIZP9LgEj8uHu4+HO8aP6inEz82y+0+Tu4bP9JuFD/2Ye0+EOwcP2E2FT/IB+0+A+odP2X+FT9Uquw+dOoeP73GFj8zNuw+U+kfP4qPFz+J0es+"
        "W+ogP7xYGD8RVus+6ushP1MiGT+I1uo+5usiP3DsGT8fZ+o+HO4jP/K2Gj+D4Ok+4e4kP9iBGz/kaek+4fElPzRNHD+t2+g+I/UmPxUZHT/tSeg+FvcnP0vl"
        "HT+OyOc+IvsoPweyHj93L+c+gv8pPyh/Hz+0kuY+kwIrP75MID+4BuY+mgcsP9oaIT+eYuU+Fw0tP2zpIT+VuuQ+GxMuP2O4Ij+dDuQ+WRcvP/CHIz/edOM+"
        "8x0wP+JXJD/0weI+AyUxPzkoJT8cC+I+EywyPzj5JT8eUeE+uTMzP5vKJj9Tk+A+xTs0P3OcJz+70d8+4UM1P+NuKD8gDd8+g0w2P8hBKT+VRN4+YFc3PxIV"
        "Kj+zYd0+eGA4PwPpKj95ktw+BWo5P2q9Kz9Rv9s+GXQ6P0eSLD9c6No+AoA7P7pnLT+U99k+eoo8P7Q9Lj8zGtk+Ppc9PxIULz+OIdg+TaI+PxjrLz/APdc+"
        "hq8/P6TCMD/RPtY+I71AP6aaMT/RO9U+HclBPz9zMj8vTtQ+MNdCP15MMz9KRdM+qOVDPwMmND92ONI+UfREPz8ANT8CKdE+LgNGPwHbNT+LFtA+IxRHP0q2"
        "Nj/F584+uCNIPymSNz99zs0+ATVJP6BuOD8Tmsw+C0VKP51LOT8He8s+HVdLPyApOj+KP8o+L2lMP0oHOz95Ask+lntNP/vlOz8iwsc+UI5OP0PFPD+EfsY+"
        "PKFPPyKlPT+sOMU+zLVQP5iFPj+Q18M+sMpRP5VmPz8uc8I+599SPyhIQD/IC8E+H/VTP2MqQT8zo78+iQpVPzUNQj8NOb4+NiBWP43wQj9ozLw+qDdXP43U"
        "Qz8PQ7s+Gk9YPyS5RD8wubk+rmZZP1KeRT9mLrg+9n9aPyeERj8rh7Y+X5lbP4NqRz9d3rQ+6rJcP4dRSD+kNLM+xM1dPyI5ST/BcbE+T+deP2QhSj9Yya8+"
        "vANgPz0KSz8x660+6x5hP67zSz/IJ6w+eTtiP7XdTD9rSqo+R1ljP2XITT+LVKg+83ZkP7yzTj81YqY+3ZVlP6mfTz/BV6Q+t7RmPy6MUD+UUKI+rtRnP0p5"
        "UT/9MqA+w/VoPw5nUj8IAJ4+lBZqP2lVUz+A05s+UDhrP1tEVD9blJk+A1xsP9MzVT85Kpc+Un9tP/IjVj/3ypQ+WaNuP6kUVz/dXpI+88hvP/cFWD/7zo8+"
        "A+9wP7r3WD+gN40+YRZyPxTqWT8sg4o+3j5zP+TcWj85uYc+3Gh0PznQWz99y4Q+o5N1P/TDXD8C04E+UcB2PwK4XT85Yn0+lu13P3WsXj/4GXc+AB55P/mg"
        "Xz8rT3A+yk96P32VYD/GbGk+7IR7P76JYT/YLWI+PL98P+F8Yj/BdFo+AAJ+PzNtYz80ZlI+S65+P6KYZD/jU1A+o8h+P378ZT/filQ+Sdl+P8NjZz+Fd1k+"
        "n+h+P8XKaD+g/14+"
    ),
}

_tables: Dict[str, np.ndarray] = {}
_device_tables: Dict[tuple, torch.Tensor] = {}


def table(name: str = "default") -> np.ndarray:
    """float32 [256, 3] colour table of ``name`` (read-only)."""
    name = "turbo" if name == "default" else name
    if name not in _tables:
        if name == "gray":
            t = np.repeat((np.arange(256, dtype=np.float32) / np.float32(255.0))[:, None], 3, axis=1)
        elif name in _B64:
            t = np.frombuffer(base64.b64decode("".join(_B64[name])), dtype="<f4").astype(np.float32).reshape(256, 3)
        else:
            raise ValueError(f"unknown colormap {name!r}; one of {', '.join(NAMES)}")
        t = np.ascontiguousarray(t)
        t.setflags(write=False)
        _tables[name] = t
    return _tables[name]


def device_table(name: str, device) -> torch.Tensor:
    """The table as a float32 [256, 3] tensor on ``device`` (uploaded once per table and device)."""
    device = torch.device(device)
    key = ("turbo" if name == "default" else name, device.type, device.index)
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(table(name).copy()).to(device)
    return _device_tables[key]

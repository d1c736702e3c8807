"""How a call with a `route=` argument is sent to the band route or the dense one: ONE planner for state posteriors, expected
counts, path sampling, k-best decoding and streaming decode.

    band, why = plan(trans, original, covers, entry, shape, index)      # is there a band, does the feature's route cover it
    band = choose(route, band, why, pays, who)                           # what `route` does with the answer

A feature hands over what is its own: its `covers` function over torbi_hip_*_band_covers, that entry's name and the call's
shape for a refusal, whether its 'auto' pays for a covered band (`pays`, from its table of measured classes through `share_within`)
and the exception type of its route-name check.
"""
import torch

from . import state, viterbi

ROUTES = ('auto', 'dense', 'band')
# the states of the matrix every table of measured classes was timed on (the reference's pitch matrix); a band's width counts
# as its share of a row
_MEASURED_STATES = 1440


def check_route(route, error=RuntimeError) -> str:
    if route not in ROUTES:
        raise error(f"route must be 'auto', 'dense' or 'band'; got {route!r}")
    return route


def stated(reach_left, reach_right, background):
    """The band a caller states, as (int, int, float)."""
    reach_left, reach_right, background = int(reach_left), int(reach_right), float(background)
    if reach_left < 0 or reach_right < 0:
        raise RuntimeError(f'reach_left and reach_right must be >= 0; got {reach_left}, {reach_right}')
    return reach_left, reach_right, background


def share_within(states: int, reach_left: int, reach_right: int, diagonals: int) -> bool:
    """The band holds at most `diagonals` / 1440 of a matrix row."""
    return (reach_left + reach_right + 1) * _MEASURED_STATES <= diagonals * states


def plan(trans: torch.Tensor, original: torch.Tensor, covers, entry: str, shape: dict, index: int = 0, look: bool = True,
         finite: str = 'finite'):
    """((reach_left, reach_right, background), '') where a band route takes the prepared device matrix `trans` (`original`:
    the caller's tensor, which the look is remembered with), else (None, the reason).  The structure is what
    `viterbi.band_over` answers -- one look per tensor version; an unseen matrix while a stream is capturing has no band --,
    the shape what the feature's `covers(*shape.values(), reach_left, reach_right, background, index)` takes.  `shape` is the
    call in the order of that function, batch=, states= and what else it asks about; `entry` names the function and `finite`
    says what a finite background has to be, both for the reason.  Without `look` only a structure that is already known
    counts: the look is a small kernel, a host synchronisation and, the first time, a device allocation."""
    states = shape['states']
    if shape['batch'] < 1:
        return None, 'the batch is empty'
    if not look:
        known = state.peek(original)
        if known is None or ('band_over', states) not in known:
            return None, 'the structure of the matrix is not known yet'
    over = viterbi.band_over(trans, original, states)
    if over is None:
        return None, ('the matrix does not hold one value outside a band that viterbi.band_over can answer for '
                      f'(states % 4 == 0, 64 <= states <= {viterbi.BAND_MAX_STATES}, reach_left + reach_right + 4 <= '
                      f'{viterbi.BAND_MAX_WINDOW}, a background that is -inf or {finite})')
    if not covers(*shape.values(), *over, index):
        asked = ', '.join(f'{name}={value}' for name, value in shape.items())
        return None, f'{entry} turns down {asked}, reach {over[0]}/{over[1]}, background {over[2]}'
    return over, ''


def choose(route: str, band, why: str, pays, who: str):
    """The band `route` takes, or None for the dense route: 'dense' never takes one, 'band' takes `band` or raises
    RuntimeError(`who`: `why`), 'auto' takes it where `pays(reach_left, reach_right, background)` says so (None: the band
    route won in every class that was measured).  A caller that must not look at the matrix under 'dense' does not ask
    for a plan there."""
    if route == 'dense':
        return None
    if route == 'band':
        if band is None:
            raise RuntimeError(f'{who}: {why}')
        return band
    return band if band is not None and (pays is None or pays(*band)) else None

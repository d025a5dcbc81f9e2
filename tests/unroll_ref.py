"""numpy restatement of the actor's unroll recorder (include/aaa.h
aaa_unroll_begin / aaa_unroll_record): two banks, the cursor pos = [t, bank,
unrolls completed, 0], the same writes in the same places and nothing else.
The GPU tests compare the kernels with it bit for bit; the emulation test
drives it with a synthetic stream."""
import numpy as np

BANK_F32 = ("logp", "rewards", "done")


def new_bank(T, Bu, frame_bytes, state_floats, core, fill_u8=0, fill_i32=0, fill_f32=0.0):
    """One bank in the layouts of aaa_unroll_bank, every element set to the given fill (a sentinel)."""
    f = np.float32(fill_f32)
    bank = dict(frames=np.full((T, Bu, frame_bytes), fill_u8, np.uint8), actions=np.full((T, Bu), fill_i32, np.int32),
                first=np.full(Bu, f, np.float32), h0=np.full((Bu, state_floats), f, np.float32),
                c0=np.full((Bu, state_floats), f, np.float32))
    for k in BANK_F32:
        bank[k] = np.full((T, Bu), f, np.float32)
    if core:
        bank["core_h0"] = np.full((Bu, core), f, np.float32)
        bank["core_c0"] = np.full((Bu, core), f, np.float32)
    return bank


def completed_unrolls(n, T):
    """The host formula for pos[2] after n steps from a zero cursor."""
    return 0 if n < T else 1 + (n - T) // (T - 1)


def clip_reward(r, c):
    """clip(reward_in): c == 0 as given, else clamped to [-c, c] with NaN kept (selects, in fp32)."""
    r = np.asarray(r, np.float32)
    if not c > 0:
        return r.copy()
    c = np.float32(c)
    return np.where(r < -c, -c, np.where(r > c, c, r)).astype(np.float32)


class UnrollRef:
    def __init__(self, T, B, Bu, b0, frame_bytes, state_floats, core=0, reward_clip=0.0, banks=None):
        assert T >= 2 and B >= 1 and b0 >= 0 and b0 + B <= Bu and state_floats % 4 == 0 and core in (0, 256)
        self.T, self.B, self.Bu, self.b0 = T, B, Bu, b0
        self.frame_bytes, self.state_floats, self.core, self.reward_clip = frame_bytes, state_floats, core, reward_clip
        self.banks = banks if banks is not None else [new_bank(T, Bu, frame_bytes, state_floats, core) for _ in (0, 1)]
        self.pos = np.zeros(4, np.int32)

    def begin(self, done_in, h, c, core_h=None, core_c=None):
        """Before the step; h, c (B, state_floats) and core_h, core_c (B, core) are changed in place."""
        t, k = int(self.pos[0]), int(self.pos[1])
        done = np.asarray(done_in, np.float32) != 0
        live = [("h0", h), ("c0", c)] + ([("core_h0", core_h), ("core_c0", core_c)] if self.core else [])
        for _, x in live:
            x[done] = 0.0   # a select: NaN rows become zero too
        dst = k if t == 0 else (1 - k if t == self.T - 1 else None)
        if dst is None:
            return
        rows = slice(self.b0, self.b0 + self.B)
        for name, x in live:
            self.banks[dst][name][rows] = x
        self.banks[dst]["first"][rows] = done.astype(np.float32)

    def record(self, frame, actions, logp, reward_in, done_in):
        """After the step; frame (B, frame_bytes) uint8, actions (B) int32, the rest (B) fp32."""
        T = self.T
        t, k, completed = int(self.pos[0]), int(self.pos[1]), int(self.pos[2])
        cur, nxt = self.banks[k], self.banks[1 - k]
        rows = slice(self.b0, self.b0 + self.B)
        cur["frames"][t, rows] = frame
        cur["actions"][t, rows] = actions
        cur["logp"][t, rows] = logp
        if t >= 1:
            cur["rewards"][t - 1, rows] = clip_reward(reward_in, self.reward_clip)
            cur["done"][t - 1, rows] = (np.asarray(done_in, np.float32) != 0).astype(np.float32)
        if t == T - 1:
            nxt["frames"][0, rows] = frame
            nxt["actions"][0, rows] = actions
            nxt["logp"][0, rows] = logp
            cur["rewards"][T - 1, rows] = 0.0
            cur["done"][T - 1, rows] = 0.0
            self.pos[:] = (1, 1 - k, completed + 1, 0)
        else:
            self.pos[0] = t + 1

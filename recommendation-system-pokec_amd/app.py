"""app.py — HTTP front end over the engine's api_cli (the serving half).

The reference's wrapper is python/app.py:1-162: a FastAPI app that starts the C++ api_cli as
a child process, waits for its READY line, and forwards one "USER <uid>" line per request
under a lock (the CLI is single-threaded; the caller serialises).  Its
routes are kept, with the same paths, parameters and JSON:

    GET /                               a small HTML page (the reference renders templates/index.html)
    GET /health                         {"status": "ok", "load_users": N}            (app.py:104-106)
    GET /api/user/{uid}                 the api_cli JSON line for "USER uid"         (app.py:108-120)
    GET /api/recommend/{kind}/{uid}?topk=20, kind in graph|collab|interest|clubs:
                                        recommendations[kind][:topk]                 (app.py:122-144)

and one route of the engine's own:

    GET /api/explain/{a}/{b}            the api_cli JSON line for "EXPLAIN a b": the breakdown of FAS(a, b)
    POST /api/match                     the api_cli JSON line for "MATCH ...": the most similar users for a
                                        profile given in the body, for a person who is not a user of the corpus:
                                        {"topk": 20, "public": 1, "gender": 0, "completion": 80, "age": 25,
                                         "region": [3, null, 27], "clubs": [ids], "friends": [ids], "exclude": [uids],
                                         "tokens": {"<column index>": [[tid, tf], ...]}}, every field optional.
                                        Text columns are token ids: callers that ran the reference's encoder, or
                                        that match on the fixed fields and clubs only (no text -> id ETL here).
    POST /api/match and /api/group also take the score window (pokec_fas.h pf_scan_window):
                                        "min_score": 0.3 (only results scoring at least that), "after": "<next>" (the
                                        "next" token of the page before: load more) and "count": true (the reply gains
                                        "total", the number of users in the window).  A reply to a body with one of
                                        them ends with "next", the token of its last result.
                                        "all": <cap> asks for the WHOLE window in one call (pokec_fas.h "Collect"): the
                                        reply's list is everyone in it, ranked, whatever topk is, and ends with
                                        "total"; a window above cap answers an empty list, "total" and "overflow": true.
    POST /api/match and /api/group      "top_clubs": <topk> adds "clubs" to the reply's recommendations: the clubs of the
                                        window's neighbours scored by their similarity (pokec_fas.h "Clubs by
                                        interest"), with names; "neighbours": <M> uses only the first M of the ranking.
                                        (In /api/match "clubs" is the profile's own club list, hence the other name.)
    GET /api/clubs/{uid}?topk=20&min_score=&neighbours=&cap=
                                        the api_cli JSON line for "CLUBS ...": club recommendations for a stored user
                                        from its most similar users, whether or not it has an adj_list row.

    POST /api/match and /api/group      "diverse": {"lambda": 0.7, "pool": 200} makes the reply's list the diverse top-k
                                        (pokec_fas.h "Diverse top-k"): the window's first `pool` users re-ranked by
                                        maximal marginal relevance, each item with its "pen"; the reply ends with
                                        "total" and "pool".  Not together with "all", "top_clubs" or "neighbours".
    GET /api/diverse/{uid}?topk=20&lam=0.7&pool=&min_score=
                                        the api_cli JSON line for "DIVERSE ...": the same for a stored user.

What differs, because the reference's file cannot run as written:
  * it has unresolved merge-conflict markers (app.py:38-42, 147-159); the start-up wait here
    is the HEAD side's 120 s;
  * its /api/recommend/* routes call `.get` on the JSONResponse that api_user returns, which
    raises, so they always answered 500; here they read the parsed JSON;
  * its send() timeout sits after a `break` and never fires; here a reader thread feeds a
    queue and a request that gets no line within `timeout` answers 500;
  * the backend is recommendation-system-pokec_amd/pokec_api_cli (csrc/api_cli.cpp, the
    engine's byte-identical api_cli), not build/api_cli.exe; pyngrok (a public tunnel) is
    not part of this build.
Configuration as the reference: config.yaml next to data/ (load_users, server.host,
server.port); POKEC_API_CLI overrides the backend executable.

    python recommendation-system-pokec_amd/app.py --root DIR      (needs a gfx950 GPU: the CLI opens the engine)
"""
import contextlib
import json
import os
import queue
import re
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CLI = os.path.join(HERE, "pokec_api_cli")
KINDS = {"graph": "graph", "collab": "collaborative", "interest": "interest", "clubs": "clubs"}


_CURSOR = re.compile(r"^[0-9a-fA-F]{8}:-?[0-9]{1,10}$")


def window_words(body):
    """The score window's words of a /api/match or /api/group body (csrc/match_line.h): min_score,
    after (a "next" token as a reply gave it), count and all (the collector's cap); ValueError on a
    field of the wrong shape."""
    words = []
    v = body.get("min_score")
    if v is not None:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError("min_score must be a number")
        words.append("min=" + repr(float(v)))
    v = body.get("after")
    if v is not None:
        if not isinstance(v, str) or not _CURSOR.match(v):
            raise ValueError("after must be the \"next\" token of an earlier reply")
        words.append("after=" + v)
    v = body.get("count", False)
    if not isinstance(v, bool):
        raise ValueError("count must be true or false")
    if v:
        words.append("count")
    v = body.get("all")
    if v is not None:
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 2**31 - 1:
            raise ValueError("all must be a cap between 1 and 2147483647")
        words.append("all=%d" % v)
    return words + club_words(body) + diverse_words(body)


def _lambda(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:  # NaN fails the comparison
        raise ValueError("lambda must be a number between 0 and 1")
    return repr(float(v))


def diverse_words(body):
    """The diverse top-k words of a /api/match or /api/group body: "diverse": {"lambda": x, "pool": m}
    (pool optional, 1 .. 1024); not together with "all", "top_clubs" or "neighbours": the reply holds one list."""
    d = body.get("diverse")
    if d is None:
        return []
    if not isinstance(d, dict) or set(d) - {"lambda", "pool"} or "lambda" not in d:
        raise ValueError("diverse must be {\"lambda\": x, \"pool\": m}")
    for other in ("all", "top_clubs", "neighbours"):
        if body.get(other) is not None:
            raise ValueError("diverse cannot be combined with " + other)
    words = ["diverse=" + _lambda(d["lambda"])]
    m = d.get("pool")
    if m is not None:
        if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 1024:
            raise ValueError("pool must be between 1 and 1024")
        words.append("pool=%d" % m)
    return words


def club_words(body):
    """The clubs-by-interest words of a /api/match or /api/group body: top_clubs (the "clubs" list's
    topk) and neighbours (M, with top_clubs only)."""
    words = []
    v = body.get("top_clubs")
    if v is not None:
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 1 << 20:
            raise ValueError("top_clubs must be between 1 and 1048576")
        words.append("topclubs=%d" % v)
    m = body.get("neighbours")
    if m is not None:
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 2**31 - 1:
            raise ValueError("neighbours must be between 0 and 2147483647")
        if v is None:
            raise ValueError("neighbours needs top_clubs")
        words.append("m=%d" % m)
    return words


def clubs_line(uid, topk=20, min_score=None, neighbours=None, cap=None):
    """The api_cli "CLUBS ..." line of GET /api/clubs/{uid}; ValueError on a value out of range."""
    for name, v, lo, hi in (("uid", uid, 0, 2**31 - 1), ("topk", topk, 0, 1 << 20), ("neighbours", neighbours, 0, 2**31 - 1),
                            ("cap", cap, 1, 2**31 - 1)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi):
            raise ValueError("%s must be between %d and %d" % (name, lo, hi))
    words = ["CLUBS", str(topk), str(uid)]
    if min_score is not None:
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or min_score != min_score:
            raise ValueError("min_score must be a number")
        words.append("min=" + repr(float(min_score)))
    if neighbours is not None:
        words.append("m=%d" % neighbours)
    if cap is not None:
        words.append("cap=%d" % cap)
    return " ".join(words)


def diverse_line(uid, topk=20, lam=0.7, pool=None, min_score=None):
    """The api_cli "DIVERSE ..." line of GET /api/diverse/{uid}; ValueError on a value out of range."""
    for name, v, lo, hi in (("uid", uid, 0, 2**31 - 1), ("topk", topk, 0, 1 << 20), ("pool", pool, 1, 1024)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi):
            raise ValueError("%s must be between %d and %d" % (name, lo, hi))
    words = ["DIVERSE", str(topk), str(uid), _lambda(lam)]
    if pool is not None:
        words.append("pool=%d" % pool)
    if min_score is not None:
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or min_score != min_score:
            raise ValueError("min_score must be a number")
        words.append("min=" + repr(float(min_score)))
    return " ".join(words)


def match_line(body):
    """The api_cli "MATCH ..." line of a POST /api/match body (csrc/match_line.h); ValueError on a
    field of the wrong shape."""
    if not isinstance(body, dict):
        raise ValueError("the body must be a JSON object")
    unknown = set(body) - {"topk", "public", "gender", "completion", "age", "region", "clubs", "friends", "exclude", "tokens",
                           "min_score", "after", "count", "all", "top_clubs", "neighbours", "diverse"}
    if unknown:
        raise ValueError("unknown field: " + sorted(unknown)[0])

    def ints(name, v):
        if not isinstance(v, (list, tuple)) or any(isinstance(x, bool) or not isinstance(x, int) for x in v):
            raise ValueError(name + " must be a list of integers")
        return ",".join(str(x) for x in v)

    words = ["MATCH", str(int(body.get("topk", 20)))]
    for key in ("public", "gender", "completion", "age"):
        if body.get(key) is not None:
            if isinstance(body[key], bool) or not isinstance(body[key], int):
                raise ValueError(key + " must be an integer")
            words.append(f"{key}={body[key]}")
    if body.get("region") is not None:
        reg = list(body["region"])
        if len(reg) > 3 or any(x is not None and (isinstance(x, bool) or not isinstance(x, int)) for x in reg):
            raise ValueError("region must be up to three integers or nulls")
        words.append("region=" + ",".join("" if x is None or x < 0 else str(x) for x in reg))
    for key in ("clubs", "friends", "exclude"):
        if body.get(key):
            words.append(f"{key}=" + ints(key, body[key]))
    for t, row in sorted((int(t), row) for t, row in (body.get("tokens") or {}).items()):
        if t < 0 or any(not isinstance(p, (list, tuple)) or len(p) != 2 for p in row):
            raise ValueError("tokens must map a column index to [[tid, tf], ...]")
        if row:
            words.append(f"c{t}=" + ",".join(ints("tokens", p).replace(",", ":") for p in row))
    return " ".join(words + window_words(body))


def group_line(body):
    """The api_cli "GROUP ..." line of a POST /api/group body {"seeds": [...], "topk": 20, "agg":
    "mean", "exclude": [...], "exclude_adj": false} and the window's fields (window_words); ValueError on a field of the wrong shape."""
    if not isinstance(body, dict):
        raise ValueError("the body must be a JSON object")
    unknown = set(body) - {"seeds", "topk", "agg", "exclude", "exclude_adj", "min_score", "after", "count", "all",
                           "top_clubs", "neighbours", "diverse"}
    if unknown:
        raise ValueError("unknown field: " + sorted(unknown)[0])

    def uids(name, v):
        if not isinstance(v, (list, tuple)) or any(isinstance(x, bool) or not isinstance(x, int) or x < 0 for x in v):
            raise ValueError(name + " must be a list of non-negative integers")
        return [str(x) for x in v]

    seeds = uids("seeds", body.get("seeds"))
    if not seeds:
        raise ValueError("seeds must name at least one user")
    agg = body.get("agg", "mean")
    if agg not in ("mean", "min", "max"):
        raise ValueError("agg must be mean, min or max")
    topk = body.get("topk", 20)
    if isinstance(topk, bool) or not isinstance(topk, int) or topk < 0:
        raise ValueError("topk must be a non-negative integer")
    if not isinstance(body.get("exclude_adj", False), bool):
        raise ValueError("exclude_adj must be true or false")
    words = ["GROUP", str(topk), agg] + seeds
    if body.get("exclude_adj", False):
        words.append("noadj")
    if body.get("exclude"):
        words.append("exclude=" + ",".join(uids("exclude", body["exclude"])))
    return " ".join(words + window_words(body))


def load_config(root):
    """config.yaml as the reference reads it (app.py:15-23); absent file = defaults."""
    cfg = {}
    p = os.path.join(root, "config.yaml")
    if os.path.exists(p):
        import yaml
        with open(p, "r", encoding="utf-8") as f:
            cfg = yaml.safe_load(f) or {}
    srv = cfg.get("server", {}) or {}
    return {"load_users": cfg.get("load_users", 100000), "host": srv.get("host", "0.0.0.0"),
            "port": int(srv.get("port", 8000))}


class ApiCli:
    """The api_cli child process (app.py:29-87): started in `root` (the CLI reads data/ and
    config/ relative to its cwd), READY awaited, one command line in, one JSON line out."""

    def __init__(self, cmd, root, ready_timeout=120.0):
        self.p = subprocess.Popen(cmd, cwd=root, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True, bufsize=1)
        self.lines = queue.Queue()
        self.log = []  # the loader's progress lines before READY
        threading.Thread(target=self._pump, args=(self.p.stdout, self.lines), daemon=True).start()
        threading.Thread(target=self._drain, args=(self.p.stderr,), daemon=True).start()
        self.lock = threading.Lock()
        self.owed = 0  # responses of timed-out requests still to arrive (skipped by the next send)
        deadline = time.time() + ready_timeout
        while True:
            line = self._next(deadline - time.time())
            if line is None:
                self.close()
                raise RuntimeError("api_cli did not signal READY: " + " | ".join(self.log[-5:]))
            if line.strip() == "READY":
                break
            self.log.append(line.rstrip("\n"))

    @staticmethod
    def _pump(stream, q):
        for line in stream:
            q.put(line)
        q.put(None)  # EOF

    @staticmethod
    def _drain(stream):
        for _ in stream:
            pass

    def _next(self, timeout):
        try:
            return self.lines.get(timeout=max(timeout, 0.0))
        except queue.Empty:
            return None

    def send(self, cmd, timeout=10.0):
        """One request: the first non-empty output line (app.py:58-77)."""
        with self.lock:
            while self.owed:  # one line per command: drop the late answers first
                line = self._next(timeout)
                if line is None:
                    raise TimeoutError("api_cli still busy with an earlier request")
                if line.strip():
                    self.owed -= 1
            try:
                self.p.stdin.write(cmd.rstrip("\n") + "\n")
                self.p.stdin.flush()
            except Exception as e:
                raise RuntimeError("failed write to api_cli: " + str(e))
            deadline = time.time() + timeout
            while True:
                line = self._next(deadline - time.time())
                if line is None:
                    if self.p.poll() is not None:
                        raise RuntimeError("api_cli closed output")
                    self.owed += 1
                    raise TimeoutError("timeout waiting for api_cli response")
                if line.strip():
                    return line.strip()

    def close(self):
        try:
            if self.p.poll() is None:
                self.p.stdin.write("EXIT\n")
                self.p.stdin.flush()
                self.p.wait(timeout=5)
        except Exception:
            pass
        if self.p.poll() is None:
            self.p.kill()
            self.p.wait()


def create_app(root, cli_cmd=None, load_users=None, ready_timeout=120.0, request_timeout=10.0):
    """The FastAPI app over an api_cli started in `root`.  cli_cmd: argv of the backend
    (default: pokec_api_cli [load_users], as app.py:31 builds it)."""
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import HTMLResponse, JSONResponse

    cfg = load_config(root)
    n = cfg["load_users"] if load_users is None else load_users
    if cli_cmd is None:
        exe = os.environ.get("POKEC_API_CLI", DEFAULT_CLI)
        if not os.path.exists(exe):
            raise RuntimeError(f"api_cli not found at {exe}. Build it first (make -C recommendation-system-pokec_amd).")
        cli_cmd = [exe, str(int(n))] if n else [exe]
    cli = ApiCli(cli_cmd, root, ready_timeout)

    @contextlib.asynccontextmanager
    async def lifespan(_app):  # the reference's shutdown hook (app.py:96-98)
        yield
        cli.close()

    app = FastAPI(title="Pokec Recommender API (MI355X engine backend)", lifespan=lifespan)
    app.state.cli = cli
    app.state.load_users = n

    @app.get("/", response_class=HTMLResponse)
    async def index():
        return ("<!doctype html><html><head><title>Pokec recommender</title></head><body>"
                f"<h1>Pokec recommender</h1><p>Loaded users: {n}</p>"
                "<p>GET /api/user/{uid}, /api/recommend/{graph|collab|interest|clubs}/{uid}?topk=20</p>"
                "<p>GET /api/explain/{a}/{b}: the per-field terms of the similarity of users a and b</p>"
                "<p>POST /api/match: the most similar users for a profile given in the body</p>"
                "</body></html>")

    @app.get("/health")
    async def health():
        return {"status": "ok", "load_users": n}

    def user_json(uid):
        return cli_json(f"USER {uid}")

    def cli_json(cmd):
        try:
            out = cli.send(cmd, request_timeout)
        except Exception as e:
            raise HTTPException(status_code=500, detail=str(e))
        try:
            return json.loads(out)
        except Exception as e:
            raise HTTPException(status_code=500, detail="invalid JSON from backend: " + str(e) + " output: " + out)

    # plain `def` routes: FastAPI runs them in its threadpool, so a request blocked on the
    # backend (cli.send waits up to request_timeout) never stalls the event loop (/health etc.)
    @app.get("/api/user/{uid}")
    def api_user(uid: int):
        return JSONResponse(user_json(uid))

    @app.get("/api/explain/{a}/{b}")
    def api_explain(a: int, b: int):
        return JSONResponse(cli_json(f"EXPLAIN {a} {b}"))

    @app.post("/api/match")
    def api_match(body: dict):
        try:
            line = match_line(body)
        except (ValueError, TypeError) as e:
            raise HTTPException(status_code=422, detail=str(e))
        return JSONResponse(cli_json(line))

    @app.post("/api/group")
    def api_group(body: dict):
        try:
            line = group_line(body)
        except (ValueError, TypeError) as e:
            raise HTTPException(status_code=422, detail=str(e))
        return JSONResponse(cli_json(line))

    @app.get("/api/clubs/{uid}")
    def api_clubs(uid: int, topk: int = 20, min_score: float = None, neighbours: int = None, cap: int = None):
        try:
            line = clubs_line(uid, topk, min_score, neighbours, cap)
        except (ValueError, TypeError) as e:
            raise HTTPException(status_code=422, detail=str(e))
        return JSONResponse(cli_json(line))

    @app.get("/api/diverse/{uid}")
    def api_diverse(uid: int, topk: int = 20, lam: float = 0.7, pool: int = None, min_score: float = None):
        try:
            line = diverse_line(uid, topk, lam, pool, min_score)
        except (ValueError, TypeError) as e:
            raise HTTPException(status_code=422, detail=str(e))
        return JSONResponse(cli_json(line))

    def recommend(kind):
        def route(uid: int, topk: int = 20):
            return user_json(uid).get("recommendations", {}).get(KINDS[kind], [])[:topk]
        route.__name__ = f"api_recommend_{kind}"
        return route

    for kind in KINDS:
        app.get(f"/api/recommend/{kind}/{{uid}}")(recommend(kind))
    return app


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.getcwd(), help="directory holding data/, config/ and config.yaml")
    args = ap.parse_args()
    cfg = load_config(args.root)
    app = create_app(args.root)
    import uvicorn
    print("Server starting: FastAPI wrapper (MI355X engine backend). Loaded users:", app.state.load_users)
    uvicorn.run(app, host=cfg["host"], port=cfg["port"], log_level="info")


if __name__ == "__main__":
    sys.exit(main())
